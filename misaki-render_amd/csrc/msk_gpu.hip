// msk_gpu.hip — implementation of the C ABI in include/msk_gpu.h (MI355X / gfx950 only).
//
// Host responsibilities of this file: scene upload + BVH build (replaces Scene::accel_init,
// src/librender/scene.cpp:201-212), area-light tables (mesh.cpp:39-48), the spiral block
// schedule (imageblock.cpp:176-247), the wavefront iteration loop, and the ordered film
// resolve.  Everything per-sample runs in the kernels of msk_kernels.h.
#include "msk_kernels.h"
#include "msk_serial.h"
#include "msk_direct.h"
#include "msk_bvh.h"
#include "msk_plan.h"
#include "msk_scene_tables.h"
#include "msk_lens_tables.h"
#include "msk_envmap.h"
#include "msk_lbvh.h"
#define MSK_WATCHDOG_SYNC
#include "msk_watchdog.h"
#include "../../include/msk_gpu.h"
#include <hip/hip_ext.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <memory>
#include <string>
#include <thread>
#include <vector>
#include <type_traits>

using namespace msk;
using mskplan::env_u32;

static thread_local std::string g_last_error;

#define MSK_MAX_GROUP 8                 /* devices behind one context (msk_multi.h) */
struct msk_group;
struct msk_ctx {
    msk_group *group = nullptr;        // non-null: a group context (msk_gpu_init with n > 1); the fields below describe its first device
    int device = 0;
    hipStream_t stream = nullptr;
    hipDeviceProp_t prop;
    std::string last_error;
#ifndef MSK_MAX_STREAMS
#define MSK_MAX_STREAMS 4
#endif
    hipStream_t more_streams[MSK_MAX_STREAMS - 1] = {};   // the other parts of the pool run here (run_wavefront)
    Ctrl *h_ctrl = nullptr;            // pinned, [MSK_MAX_STREAMS]: one per part
    std::vector<hipEvent_t> events, more_events[MSK_MAX_STREAMS - 1];
    uint32_t timing_phase = 0;         // which sync groups carry timing events rotates from render to render (MSK_TIMING_EVERY);
                                       // a context is used by one host thread at a time (msk_gpu.h), so a plain counter
    bool lost = false;                 // the watchdog gave up on a render (msk_watchdog.h): every later call fails at once, shutdown releases host memory only
    mskwd::Hub *hub = nullptr;         // what the host functions of MSK_WAIT=callback signal; leaked with a lost context (msk_watchdog.h)
    hipEvent_t wait_events[MSK_MAX_STREAMS] = {};      // MSK_WAIT=event: hipEventBlockingSync events, one per part of the pool
    uint32_t device_sharers = 1;       // member contexts of a group that sit on this context's device (repeated ordinals): their
                                       // renders run side by side, each plans its record buffers within 1 / device_sharers of the free HBM
};

static int fail(msk_ctx *ctx, int code, const char *fmt, ...) {
    char buf[1024];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
    g_last_error = buf;
    if (ctx) ctx->last_error = buf;
    return code;
}
// The same for code that runs on the helper threads of a render (run_wavefront): the text goes to a slot the thread
// owns; the calling thread copies the first failure into the context after the join.  ctx->last_error is only ever
// written by the thread that called into the library.
static int fail_to(std::string *slot, int code, const char *fmt, ...) {
    char buf[1024];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
    *slot = buf;
    return code;
}
// what a failed runtime call becomes in the ABI: the one place that tells the two codes apart
static int hip_code(hipError_t e) { return e == hipErrorOutOfMemory ? MSK_ERR_OOM : MSK_ERR_HIP; }
#define HIP_TRY_SLOT(slot, expr)                                                                 \
    do { hipError_t e_ = (expr); if (e_ != hipSuccess)                                          \
        return fail_to(slot, hip_code(e_), "%s failed: %s (%s:%d)", #expr, \
                       hipGetErrorString(e_), __FILE__, __LINE__); } while (0)
#define HIP_TRY(ctx, expr)                                                                       \
    do { hipError_t e_ = (expr); if (e_ != hipSuccess)                                          \
        return fail(ctx, hip_code(e_), "%s failed: %s (%s:%d)", #expr, \
                    hipGetErrorString(e_), __FILE__, __LINE__); } while (0)

// a context the watchdog gave up on (msk_watchdog.h): nothing runs on it any more
#define MSK_REFUSE_LOST(ctx) do { if ((ctx) && (ctx)->lost) return fail(ctx, MSK_ERR_HIP, "this context is lost: an earlier render made no progress " \
                                                                         "(msk_watchdog.h); shut it down and start over in a new process"); } while (0)
struct DevBuf {
    void *p = nullptr; size_t bytes = 0;
    ~DevBuf() { if (p) (void) hipFree(p); }
    hipError_t alloc(size_t n) { if (p) (void) hipFree(p); p = nullptr; bytes = n; return n ? hipMalloc(&p, n) : hipSuccess; }
    hipError_t reserve(size_t n) { return (p && bytes >= n) ? hipSuccess : alloc(n); }     // grow-only (workspace reuse)
    template <typename T> hipError_t upload(const std::vector<T> &v) {
        hipError_t e = reserve(std::max<size_t>(v.size() * sizeof(T), 16));
        if (e != hipSuccess) return e;
        return v.empty() ? hipSuccess : hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
    }
    template <typename T> T *as() const { return (T *) p; }
    void leak() { p = nullptr; bytes = 0; }        // a lost context: hipFree would wait for a kernel that never finishes; the memory goes with the process
};

struct Workspace;
struct msk_scene {
    msk_ctx *ctx = nullptr;
    // a scene of a group context: one ordinary scene per member, the members' films, staging copies for members without
    // peer access, and the summed film (msk_multi.h); everything below `ws` is then unused but dev.width / dev.height
    std::vector<msk_scene *> parts;
    DevBuf part_films[MSK_MAX_GROUP], staged[MSK_MAX_GROUP], group_film;
    void *group_host_film = nullptr; size_t group_host_film_bytes = 0;      // pinned staging of a group's copy-back (film_to_host)
    Workspace *ws = nullptr;           // render buffers, kept between calls (hipMalloc/hipFree of GBs costs milliseconds)
    DeviceScene dev;
    DevBuf nodes, nodes4, nodes4q, nodes8, tris, tris3, tri_bounds, tri_verts, tri_frames, tri_normals, tri_uvs, mesh_info, bsdfs, emitters, emitter_d65, emitter_grid, spectra, texels, cdf, cie;
    mskplan::SceneFacts facts;         // what the scene holds, which tree the traversal kernels walk and where tree and tables live: decided once, at
                                       // creation (msk_scene_tables.h, msk_plan.h), and all a render's launch plan needs to know of the scene
    std::vector<int32_t> emitter_types, bsdf_types;      // msk_gpu_point_sample / msk_gpu_conductor_sample check their index against these
    std::vector<float> plastic_constants;                // {fdr_int, ssw} per BSDF entry of a scene that holds a plastic (msk_gpu_plastic_constants)
    uint32_t n_textures = 0, tex_base = 0;      // msk_gpu_eval_texture: texture k's record sits at float4 tex_base + 3 k of `bsdfs`
    int bvh_depth = 0;
    uint32_t n_tris = 0;
};

static int ctx_sync(msk_ctx *ctx, hipStream_t stream, const char *what, double limit_scale = 1.0);     // (below: every wait of a render is timed)
static int film_to_host(msk_ctx *ctx, hipStream_t stream, const void *d_film, float *h_film, size_t bytes, void **stage, size_t *stage_bytes);
#include "msk_multi.h"

#ifdef MSK_COUNT
// instrumented builds only: reads and clears the traversal counters of msk_kernels.h
extern "C" int msk_gpu_debug_counts(unsigned long long *out16) {
    unsigned long long z[16] = {};
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpyFromSymbol(out16, HIP_SYMBOL(msk_counts), sizeof z) != hipSuccess) return -1;
    return hipMemcpyToSymbol(HIP_SYMBOL(msk_counts), z, sizeof z) == hipSuccess ? 0 : -1;
}
#endif
// ------------------------------------------------------------------------------------------
extern "C" const char *msk_gpu_last_error(const msk_ctx *ctx) {
    return ctx ? ctx->last_error.c_str() : g_last_error.c_str();
}

extern "C" int msk_gpu_init(const int *device_ids, int n, msk_ctx **out_ctx) {
    if (!out_ctx) return fail(nullptr, MSK_ERR_INVALID_ARG, "msk_gpu_init: out_ctx is NULL");
    *out_ctx = nullptr;
    if (n < 1 || !device_ids)
        return fail(nullptr, MSK_ERR_INVALID_ARG, "msk_gpu_init: at least one device per context (got n=%d)", n);
    if (n > 1) return group_init(device_ids, n, out_ctx);          // msk_multi.h: one member context per entry
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count == 0)
        return fail(nullptr, MSK_ERR_NO_DEVICE, "msk_gpu_init: no HIP device visible");
    if (device_ids[0] < 0 || device_ids[0] >= count)
        return fail(nullptr, MSK_ERR_INVALID_ARG, "msk_gpu_init: device %d out of range (0..%d)", device_ids[0], count - 1);
    msk_ctx *ctx = new msk_ctx();
    ctx->device = device_ids[0];
    hipError_t e = hipSetDevice(ctx->device);
    if (e == hipSuccess) e = hipGetDeviceProperties(&ctx->prop, ctx->device);
    // The library's streams and the process's other streams.  The HIP runtime maps streams onto a few hardware queues PER PRIORITY
    // LEVEL (GPU_MAX_HW_QUEUES, default 4); streams beyond that share a queue and their launches serialise.  In a process that also
    // runs torch and RCCL (bench.py's ranks: torch's stream, the communicator's streams) two of the four wavefront loops ended up
    // behind each other: the N > 1 step took 39.4 ms against the 32.5 of the same render in a plain process (round 6,
    // profiles/r06_hw_queues.txt) — a fifth of the weak-scaling budget before any GPU talks to another.  MSK_STREAM_PRIORITY = high
    // (default) creates the library's streams at the device's highest stream priority: their own pool of hardware queues, which
    // nothing else in the process uses; normal / low: priority 0 / the lowest (then raise GPU_MAX_HW_QUEUES in the environment).
    int prio = 0;
    {
        int least = 0, greatest = 0;
        const char *ps = getenv("MSK_STREAM_PRIORITY");
        if (e == hipSuccess && hipDeviceGetStreamPriorityRange(&least, &greatest) == hipSuccess)
            prio = (!ps || !strcmp(ps, "high")) ? greatest : !strcmp(ps, "low") ? least : 0;
        (void) hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamCreateWithPriority(&ctx->stream, hipStreamNonBlocking, prio);
    for (int k = 0; k < MSK_MAX_STREAMS - 1; ++k) if (e == hipSuccess) e = hipStreamCreateWithPriority(&ctx->more_streams[k], hipStreamNonBlocking, prio);
    if (e == hipSuccess) e = hipHostMalloc((void **) &ctx->h_ctrl, MSK_MAX_STREAMS * sizeof(Ctrl), hipHostMallocDefault);
    ctx->hub = new mskwd::Hub();
    for (int k = 0; k < MSK_MAX_STREAMS; ++k) if (e == hipSuccess) e = hipEventCreateWithFlags(&ctx->wait_events[k], hipEventBlockingSync | hipEventDisableTiming);
    if (e != hipSuccess) {
        int rc = fail(nullptr, MSK_ERR_HIP, "msk_gpu_init: %s", hipGetErrorString(e));
        msk_gpu_shutdown(ctx);             // releases whichever of stream / pinned block exist
        return rc;
    }
    if (std::string(ctx->prop.gcnArchName).find("gfx950") == std::string::npos &&
        !getenv("MSK_ALLOW_ANY_ARCH")) {
        int rc = fail(nullptr, MSK_ERR_UNSUPPORTED, "msk_gpu_init: device is %s, this library is built for gfx950 only",
                      ctx->prop.gcnArchName);
        msk_gpu_shutdown(ctx);
        return rc;
    }
    *out_ctx = ctx;
    return MSK_OK;
}

extern "C" void msk_gpu_shutdown(msk_ctx *ctx) {
    if (!ctx) return;
    if (ctx->group) { group_shutdown(ctx); return; }
    if (ctx->lost) { delete ctx; return; }          // a stream that holds a kernel which never finished: destroying it would wait for it
                                                    // (ctx->hub stays: a host function queued behind that kernel may still fire)
    (void) hipSetDevice(ctx->device);
    for (auto ev : ctx->events) (void) hipEventDestroy(ev);
    for (auto ev : ctx->wait_events) if (ev) (void) hipEventDestroy(ev);
    for (int k = 0; k < MSK_MAX_STREAMS - 1; ++k) {
        for (auto ev : ctx->more_events[k]) (void) hipEventDestroy(ev);
        if (ctx->more_streams[k]) (void) hipStreamDestroy(ctx->more_streams[k]);
    }
    if (ctx->h_ctrl) (void) hipHostFree(ctx->h_ctrl);
    if (ctx->stream) (void) hipStreamDestroy(ctx->stream);      // (waits for what the stream holds: every host function has fired)
    delete ctx->hub;
    delete ctx;
}

extern "C" int msk_gpu_describe(const msk_ctx *ctx, char *buf, uint64_t buf_size) {
    if (!ctx || !buf || !buf_size) return fail(nullptr, MSK_ERR_INVALID_ARG, "msk_gpu_describe: bad argument");
    if (ctx->group) {
        char one[512];
        msk_gpu_describe(ctx->group->ctxs[0], one, sizeof one);
        std::string ids;
        for (msk_ctx *c : ctx->group->ctxs) ids += (ids.empty() ? "" : ",") + std::to_string(c->device);
        snprintf(buf, (size_t) buf_size, "%zu devices [%s], sample-sharded, film summed on device %d; each: %s", ctx->group->ctxs.size(), ids.c_str(), ctx->device, one);
        return MSK_OK;
    }
    snprintf(buf, (size_t) buf_size, "%s (%s), %d CUs, %.1f GiB HBM, LDS/block %zu KiB; libmsk_gpu ABI %d, fp-contract off; host side: "
             "%u loop thread(s) per render, wait = %s",
             ctx->prop.name, ctx->prop.gcnArchName, ctx->prop.multiProcessorCount,
             ctx->prop.totalGlobalMem / 1073741824.0, ctx->prop.sharedMemPerBlock / 1024, MSK_ABI_VERSION,
             std::max(1u, env_u32("MSK_HOST_THREADS", 1)), mskwd::wait_mode_name(mskwd::wait_mode_from_env()));
    return MSK_OK;
}

// ------------------------------------------------------------------------------------------
// scene: msk_scene_tables.h checks the descriptor and packs the tables, msk_plan.h reads the knobs and places tree and tables;
// what is left here is the device side — upload, the device-built tree, DeviceScene, the two preparation kernels
// ------------------------------------------------------------------------------------------
// The tables, and the host-built tree (host_tree; nullptr = room for the device-built one instead).
static int upload_tables(msk_scene *s, const mskscene::HostTables &t, const mskbvh::Built *host_tree, size_t n_faces) {
    hipError_t e = hipSuccess;
    auto up = [&](DevBuf &b, const std::vector<float> &v) { if (e == hipSuccess) e = b.upload(v); };
    if (host_tree) { up(s->nodes, host_tree->nodes); up(s->tris, host_tree->tris); up(s->tri_bounds, host_tree->bounds); }
    up(s->tri_verts, t.tv); up(s->tri_normals, t.tn); up(s->tri_uvs, t.tuv);
    up(s->bsdfs, t.bsdfs); up(s->emitters, t.emitters); up(s->emitter_d65, t.d65); up(s->cdf, t.cdf_all); up(s->cie, t.cie);
    up(s->emitter_grid, t.emitter_grid); up(s->spectra, t.spectra_pool);
    if (t.has_bitmap || t.has_envmap || t.has_mask_image) up(s->texels, t.texels);
    if (e == hipSuccess) e = s->mesh_info.upload(t.mesh_info);
    if (e == hipSuccess && !host_tree)
        if ((e = s->nodes.alloc(n_faces * 64)) == hipSuccess && (e = s->tris.alloc(n_faces * 64)) == hipSuccess) e = s->tri_bounds.alloc(n_faces * 32);
    return e == hipSuccess ? MSK_OK : fail(s->ctx, hip_code(e), "scene upload: %s", hipGetErrorString(e));
}

// MSK_BVH_BUILD=gpu: a linear BVH from the uploaded vertices (msk_lbvh.hip).  The node records come back to the host: the
// placement's bookkeeping and the wide collapse read them.
static int device_build_tree(msk_scene *s, const mskscene::HostTables &t, const msk_scene_desc *d, const mskplan::SceneKnobs &knobs, mskbvh::Built *bvh) {
    msk_ctx *ctx = s->ctx;
    msklbvh::Input in;
    in.tri_verts = s->tri_verts.as<float4>(); in.n_tris = d->n_faces;
    for (int k = 0; k < 3; ++k) { in.lo[k] = t.scene_lo[k]; in.hi[k] = t.scene_hi[k]; }
    in.box_pad = 2.f * t.tri_pad; in.tri_pad = t.tri_pad;
    in.leaf_size = knobs.bvh_leaf;
    in.mesh_info = s->mesh_info.as<int4>(); in.bsdfs = s->bsdfs.as<float4>(); in.n_bsdfs = d->n_bsdfs; in.bsdf_f4 = MSK_BSDF_F4;
    in.class_shift = t.all_diffuse ? 0u : (uint32_t) MSK_CLASS_SHIFT;
    msklbvh::Result res;
    char msg[256] = "";
    if (msklbvh::build(ctx->stream, in, s->nodes.as<float4>(), s->tris.as<float4>(), s->tri_bounds.as<float4>(), &res, msg, sizeof msg))
        return fail(ctx, MSK_ERR_HIP, "device BVH build: %s", msg);
    bvh->root_ref = res.root_ref; bvh->max_depth = res.depth;
    bvh->nodes.resize((size_t) res.n_nodes * 16);
    if (res.n_nodes) {
        hipError_t ec = hipMemcpy(bvh->nodes.data(), s->nodes.p, (size_t) res.n_nodes * 64, hipMemcpyDeviceToHost);
        if (ec != hipSuccess) return fail(ctx, MSK_ERR_HIP, "device BVH build: %s", hipGetErrorString(ec));
    }
    return MSK_OK;
}

// The form of the tree the placement chose, next to the binary one; for the 4-wide forms in HBM also the three-load triangle
// records, packed on the device from `tris`.  (A failure here is reported as MSK_ERR_OOM whatever the runtime said, where
// upload_tables tells MSK_ERR_HIP from MSK_ERR_OOM: kept as it always was.)
static int upload_tree_form(msk_scene *s, const mskbvh::Built &bvh, int trace_mode, uint32_t n_faces) {
    msk_ctx *ctx = s->ctx;
    hipError_t e = hipSuccess;
    switch (trace_mode) {
    case mskplan::TRACE_WIDE8: e = s->nodes8.upload(bvh.nodes8); break;
    case mskplan::TRACE_WIDE4_LDS: e = s->nodes4.upload(bvh.nodes4); break;
    case mskplan::TRACE_WIDE4: case mskplan::TRACE_WIDE4_BYTE: case mskplan::TRACE_WIDE4_HALF:
        // the traversal addresses nodes and triangle records through buffer resources with 32-bit byte offsets
        if ((uint64_t) (bvh.nodes4.size() / 32) * 128u >= (1ull << 32) || (uint64_t) n_faces * MSK_TRI_REC_BYTES >= (1ull << 32))
            return fail(ctx, MSK_ERR_UNSUPPORTED, "a tree of %zu 4-wide nodes exceeds the 4 GB a buffer resource addresses", bvh.nodes4.size() / 32);
        e = s->nodes4.upload(bvh.nodes4);
        if (e == hipSuccess && trace_mode != mskplan::TRACE_WIDE4) e = s->nodes4q.upload(trace_mode == mskplan::TRACE_WIDE4_HALF ? bvh.nodes4h : bvh.nodes4q);
        if (e == hipSuccess) e = s->tris3.alloc(std::max<size_t>((size_t) n_faces * MSK_TRI_REC_BYTES, 16));
        if (e == hipSuccess && n_faces)
            hipLaunchKernelGGL(k_pack_tris3, dim3((n_faces + MSK_BLOCK - 1) / MSK_BLOCK), dim3(MSK_BLOCK), 0, ctx->stream,
                               s->tris.as<float4>(), s->tri_bounds.as<float4>(), n_faces, s->tris3.as<float4>());
        break;
    default: break;                 // the binary tree: uploaded with the tables
    }
    return e == hipSuccess ? MSK_OK : fail(ctx, MSK_ERR_OOM, "scene upload: %s", hipGetErrorString(e));
}

// DeviceScene, whole: the uploaded tables, the tree as placed, the descriptor's camera and film.
static void fill_device_scene(msk_scene *s, const mskscene::HostTables &t, const msk_scene_desc *d, const mskbvh::Built &bvh, uint32_t n_nodes,
                              const mskbvh::CullBounds &cb, const mskplan::TreePlacement &tree) {
    DeviceScene &ds = s->dev;
    std::memset(&ds, 0, sizeof ds);
    ds.nodes = s->nodes.as<float4>(); ds.tris = s->tris.as<float4>(); ds.tri_bounds = s->tri_bounds.as<float4>(); ds.tri_pad = t.tri_pad; ds.tri_verts = s->tri_verts.as<float4>();
    ds.tri_normals = t.any_normals ? s->tri_normals.as<float4>() : nullptr;
    ds.tri_uvs = t.any_uvs ? s->tri_uvs.as<float4>() : nullptr;
    ds.tri_frames = s->tri_frames.as<float4>();
    ds.mesh_info = s->mesh_info.as<int4>(); ds.bsdfs = s->bsdfs.as<float4>(); ds.emitters = s->emitters.as<float4>();
    ds.emitter_d65 = s->emitter_d65.as<float>(); ds.cdf = s->cdf.as<float>(); ds.cie = s->cie.as<float>();
    ds.emitter_grid = s->emitter_grid.as<float4>(); ds.spectra = s->spectra.as<float>(); ds.n_spectra = d->n_regular_values;
    ds.texels = (t.has_bitmap || t.has_envmap || t.has_mask_image) ? s->texels.as<float4>() : nullptr;
    ds.n_nodes = n_nodes; ds.n_tris = d->n_faces; ds.n_emitters = d->n_emitters;
    ds.n_meshes = d->n_meshes; ds.n_bsdfs = d->n_bsdfs; ds.n_bsdf_f4 = t.n_bsdf_f4; ds.cdf_len = (uint32_t) t.cdf_all.size();
    ds.root_ref = bvh.root_ref;
    switch (tree.trace_mode) {
    case mskplan::TRACE_WIDE8:
        ds.nodes8 = s->nodes8.as<float4>(); ds.root_ref8 = bvh.root_ref8; ds.n_nodes8 = (uint32_t) (bvh.nodes8.size() / 32);
        break;
    case mskplan::TRACE_WIDE4: case mskplan::TRACE_WIDE4_BYTE: case mskplan::TRACE_WIDE4_HALF: case mskplan::TRACE_WIDE4_LDS:
        ds.nodes4 = s->nodes4.as<float4>(); ds.root_ref4 = bvh.root_ref4; ds.n_nodes4 = (uint32_t) (bvh.nodes4.size() / 32);
        if (tree.trace_mode == mskplan::TRACE_WIDE4_LDS) break;
        if (tree.trace_mode != mskplan::TRACE_WIDE4) ds.nodes4q = s->nodes4q.as<float4>();
        if (tree.trace_mode == mskplan::TRACE_WIDE4_HALF && !(ds.root_ref4 & MSK_LEAF_BIT)) ds.root_ref4 *= 80u;     // inner references of this form are byte offsets (msk_bvh.h: quantise_h)
        ds.tris3 = s->tris3.as<float4>();
        break;
    default: break;
    }
    ds.stack_entries = tree.stack_entries; ds.stack_total = tree.stack_total;
    std::memcpy(ds.s2c, d->camera.sample_to_camera, 64); std::memcpy(ds.to_world, d->camera.to_world, 64);
    ds.near_clip = d->camera.near_clip; ds.far_clip = d->camera.far_clip;
    ds.width = d->film.width; ds.height = d->film.height;
    ds.crop_x = d->film.crop_offset[0]; ds.crop_y = d->film.crop_offset[1];
    ds.crop_w = d->film.crop_size[0]; ds.crop_h = d->film.crop_size[1];
    if (ds.crop_w == 0 && ds.crop_h == 0) { ds.crop_x = ds.crop_y = 0; ds.crop_w = ds.width; ds.crop_h = ds.height; }      // the whole film
    ds.filter_radius = d->film.filter_radius;
    ds.filter_scale = float(MSK_FILTER_RESOLUTION) / d->film.filter_radius;           // rfilter.cpp:21
    ds.filter_border = (int) std::ceil(d->film.filter_radius - .5f);                  // rfilter.cpp:22
    std::memcpy(ds.lut, d->film.filter_lut, sizeof ds.lut);
    ds.env_emitter = t.env_emitter; ds.env_radius = t.env_radius;
    // the bounds a camera ray must meet (msk_bvh.h: cull_bounds)
    for (int k = 0; k < 3; ++k) { ds.cull_lo[k] = cb.lo[k]; ds.cull_hi[k] = cb.hi[k]; }
}

extern "C" int msk_gpu_scene_create(msk_ctx *ctx, const msk_scene_desc *d, msk_scene **out) { return msk_gpu_scene_create_env(ctx, d, nullptr, out); }
extern "C" int msk_gpu_scene_create_env(msk_ctx *ctx, const msk_scene_desc *d, const msk_envmap_desc *env, msk_scene **out) {
    const msk_scene_ext ext = {env, 0u, nullptr};
    return msk_gpu_scene_create_ext(ctx, d, &ext, out);
}
extern "C" int msk_gpu_scene_create_ext(msk_ctx *ctx, const msk_scene_desc *d, const msk_scene_ext *ext, msk_scene **out) {
    msk_scene_masks em = {{nullptr, 0u, nullptr}, 0u, nullptr};
    if (ext) em.ext = *ext;
    return msk_gpu_scene_create_masks(ctx, d, &em, out);
}
extern "C" int msk_gpu_scene_create_masks(msk_ctx *ctx, const msk_scene_desc *d, const msk_scene_masks *em, msk_scene **out) {
    msk_scene_lights el = {{{nullptr, 0u, nullptr}, 0u, nullptr}, 0u, nullptr};
    if (em) el.masks = *em;
    return msk_gpu_scene_create_lights(ctx, d, &el, out);
}
extern "C" int msk_gpu_scene_create_lights(msk_ctx *ctx, const msk_scene_desc *d, const msk_scene_lights *el, msk_scene **out) {
    msk_scene_lens ln = {{{{nullptr, 0u, nullptr}, 0u, nullptr}, 0u, nullptr}, nullptr};
    if (el) ln.lights = *el;
    return msk_gpu_scene_create_lens(ctx, d, &ln, out);
}
extern "C" int msk_gpu_scene_create_lens(msk_ctx *ctx, const msk_scene_desc *d, const msk_scene_lens *eln, msk_scene **out) {
    const msk_scene_lights *el = eln ? &eln->lights : nullptr;
    const msk_lens_desc *lens = eln ? eln->lens : nullptr;
    const msk_scene_masks *em = el ? &el->masks : nullptr;
    const msk_scene_ext *ext = em ? &em->ext : nullptr;
    if (!ctx || !d || !out) return fail(ctx, MSK_ERR_INVALID_ARG, "msk_gpu_scene_create: NULL argument");
    *out = nullptr;
    MSK_REFUSE_LOST(ctx);
    if (ctx->group) return group_scene_create(ctx, d, eln, out);
    const mskplan::SceneKnobs knobs = mskplan::read_scene_knobs();
    mskscene::HostTables t;
    {
        std::string msg;
        if (int rc = mskscene::pack(d, ext, knobs.pad_scale, &t, &msg, em ? em->n_masks : 0u, em ? em->masks : nullptr, el ? el->n_lights : 0u,
                                     el ? el->lights : nullptr)) return fail(ctx, rc, "%s", msg.c_str());
        if (int rc = mskscene::check_lens(lens, &msg)) return fail(ctx, rc, "%s", msg.c_str());
        if (lens) mskscene::add_lens_tables(d, &t);      // (msk_lens_tables.h: the lens kernels carry the mask code)
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));

    const bool gpu_build = knobs.gpu_build && d->n_faces > 0;
    mskbvh::Built bvh;
    if (!gpu_build) {
        bvh = mskbvh::build(t.pos.data(), d->n_faces, t.tri_pad);
        // (all_diffuse is the packer's final flag: an environment or point emitter clears it in a scene whose BSDFs are all plain
        // diffuse — every class is then 0 and tagging changes no bit, here as in msk_lbvh.hip's class_shift branch)
        if (!t.all_diffuse) mskscene::tag_classes(bvh, t, d);
    }
    std::unique_ptr<msk_scene> s(new msk_scene());
    s->ctx = ctx; s->n_tris = d->n_faces;
    s->emitter_types = std::move(t.emitter_types); s->bsdf_types = std::move(t.bsdf_types);
    if (t.has_plastic) {                                   // msk_gpu_plastic_constants: words 5 and 6 of every BSDF record (a roughplastic's: 20 and 21)
        s->plastic_constants.resize((size_t) d->n_bsdfs * 2);
        for (uint32_t b = 0; b < d->n_bsdfs; ++b) {
            const float *o = &t.bsdfs[(size_t) b * 4 * MSK_BSDF_F4 + mskscene::plastic_constants_word(s->bsdf_types[b])];
            s->plastic_constants[b * 2] = o[0]; s->plastic_constants[b * 2 + 1] = o[1];
        }
    }
    s->n_textures = t.n_textures; s->tex_base = t.tex_base;
    if (int rc = upload_tables(s.get(), t, gpu_build ? nullptr : &bvh, d->n_faces)) return rc;
    if (gpu_build) if (int rc = device_build_tree(s.get(), t, d, knobs, &bvh)) return rc;
    s->bvh_depth = bvh.max_depth;                          // (k_path_serial sizes its stack by it)

    // the camera cull's bounds: the binary tree's root, host- or device-built, before any collapse.  With an environment emitter
    // a ray that leaves the scene carries radiance: nothing is culled
    const mskbvh::CullBounds cb = mskbvh::cull_bounds(bvh.nodes, bvh.root_ref, d->n_faces);
    mskplan::BinaryTree binary;
    binary.n_nodes = (uint32_t) (bvh.nodes.size() / 16); binary.n_tris = d->n_faces; binary.max_depth = bvh.max_depth; binary.root_is_leaf = (bvh.root_ref & MSK_LEAF_BIT) != 0;
    const mskplan::TreePlacement tree = mskplan::place_tree(binary, knobs, [&](int width) {
        mskplan::WideTree w;
        if (width == 8) { w.ok = mskbvh::collapse8(bvh); w.max_depth = bvh.max_depth8; w.n_nodes = (uint32_t) (bvh.nodes8.size() / 32); }
        else {
            mskbvh::collapse4(bvh, knobs.collapse_optimal);
            w.ok = true; w.max_depth = bvh.max_depth4; w.n_nodes = (uint32_t) (bvh.nodes4.size() / 32); w.has_half = !bvh.nodes4h.empty(); w.has_byte = !bvh.nodes4q.empty();
        }
        return w;
    });
    if (int rc = upload_tree_form(s.get(), bvh, tree.trace_mode, d->n_faces)) return rc;
    mskplan::TableCounts counts;
    counts.n_tris = d->n_faces; counts.n_meshes = d->n_meshes; counts.n_bsdf_f4 = t.n_bsdf_f4; counts.n_emitters = d->n_emitters;
    counts.cdf_len = (uint32_t) t.cdf_all.size(); counts.n_spectra = d->n_regular_values;
    const mskplan::TablePlacement tables = mskplan::place_tables(counts);
    mskplan::SceneFacts &f = s->facts;
    f.trace_mode = tree.trace_mode; f.lds_scene = tree.lds_scene; f.trace_lds_bytes = tree.trace_lds_bytes;
    f.lds_tables = tables.lds_tables; f.shade_lds_bytes = tables.shade_lds_bytes;
    f.all_diffuse = t.all_diffuse; f.has_regular = t.has_regular; f.has_dielectric = t.has_dielectric; f.has_bitmap = t.has_bitmap;
    f.has_envmap = t.has_envmap; f.has_delta = t.has_delta; f.has_mask = t.has_mask; f.has_plastic = t.has_plastic; f.has_lens = lens != nullptr;
    f.cull_ok = cb.on && t.env_emitter < 0;
    if (f.trace_lds_bytes > ctx->prop.sharedMemPerBlock)
        return fail(ctx, MSK_ERR_UNSUPPORTED, "BVH depth %d needs %zu B of traversal stack per block", bvh.max_depth, tree.binary_stack_bytes);

    // per-triangle shading constants, computed on the device by the code the per-hit path used to run (k_tri_frames)
    hipError_t ef = s->tri_frames.alloc(std::max<size_t>((size_t) d->n_faces * 48, 16));
    if (ef != hipSuccess) return fail(ctx, MSK_ERR_OOM, "scene upload: %s", hipGetErrorString(ef));
    fill_device_scene(s.get(), t, d, bvh, binary.n_nodes, cb, tree);
    if (lens) { s->dev.lens_radius = lens->aperture_radius; s->dev.focus_distance = lens->focus_distance; }
    if (d->n_faces) {
        hipLaunchKernelGGL(k_tri_frames, dim3((d->n_faces + MSK_BLOCK - 1) / MSK_BLOCK), dim3(MSK_BLOCK), 0, ctx->stream, s->dev, s->tri_frames.as<float4>());
        ef = hipStreamSynchronize(ctx->stream);
        if (ef != hipSuccess) return fail(ctx, MSK_ERR_HIP, "k_tri_frames: %s", hipGetErrorString(ef));
    }
    *out = s.release();
    return MSK_OK;
}

void free_workspace(msk_scene *scene);
extern "C" void msk_gpu_scene_destroy(msk_scene *scene) {
    if (!scene) return;
    if (scene->ctx->group) { group_scene_destroy(scene); return; }
    if (scene->ctx->lost) return;         // hipFree waits for the device: under a kernel that never finished it would wait for ever; the memory goes with the process
    (void) hipSetDevice(scene->ctx->device);
    free_workspace(scene);
    delete scene;
}

// ------------------------------------------------------------------------------------------
// spiral block schedule — BlockGenerator (imageblock.cpp:176-247)
// ------------------------------------------------------------------------------------------
struct HostBlock { int off_x, off_y, size_x, size_y, bx, by; };
static std::vector<HostBlock> spiral_blocks(int w, int h, int bs, int *nbx, int *nby) {
    const int bx = (int) std::ceil(w / (float) bs), by = (int) std::ceil(h / (float) bs);
    *nbx = bx; *nby = by;
    const int count = bx * by;
    std::vector<HostBlock> out;
    out.reserve(count);
    int dir = 0, px = bx / 2, py = by / 2, steps_left = 1, steps = 1;
    for (int counter = 0; counter < count;) {
        const int ox = px * bs, oy = py * bs;
        out.push_back(HostBlock{ox, oy, std::min(w - ox, bs), std::min(h - oy, bs), px, py});
        ++counter;
        if (counter == count) break;
        do {
            switch (dir) { case 0: ++px; break; case 1: ++py; break; case 2: --px; break; default: --py; break; }
            if (--steps_left == 0) {
                dir = (dir + 1) % 4;
                if (dir == 2 || dir == 0) ++steps;
                steps_left = steps;
            }
        } while (px < 0 || py < 0 || px >= bx || py >= by);
    }
    return out;
}

// ------------------------------------------------------------------------------------------
// wavefront driver
// ------------------------------------------------------------------------------------------
struct StateBufs {
    DevBuf id, wl, thr, res, ray_o, ray_d, sh, contrib, hit, aux, counts, ctrl, stack_ovf[MSK_MAX_STREAMS];
    PathState st;
    hipError_t alloc(size_t n, uint32_t n_regions) {      // n = slots a sweep can hold live; every region has two halves of them
        hipError_t e;
#define A_(b, sz) if ((e = b.reserve(2 * n * (sz))) != hipSuccess) return e;
        A_(id, 8) A_(wl, 16) A_(thr, 16) A_(res, 16) A_(ray_o, 16) A_(ray_d, 16) A_(sh, 16) A_(contrib, 16) A_(hit, 16)
        A_(aux, 8)
#undef A_
        if ((e = counts.reserve((size_t) n_regions * sizeof(RegionCtl))) != hipSuccess) return e;
        if ((e = ctrl.reserve(MSK_MAX_STREAMS * sizeof(Ctrl))) != hipSuccess) return e;
        st.id = id.as<uint2>(); st.wl = wl.as<float4>(); st.thr = thr.as<float4>(); st.res = res.as<float4>();
        st.ray_o = ray_o.as<float4>(); st.ray_d = ray_d.as<float4>(); st.sh = sh.as<float4>();
        st.contrib = contrib.as<float4>(); st.hit = hit.as<float4>(); st.aux = aux.as<float2>();
        return hipSuccess;
    }
    void leak() { for (DevBuf *b : {&id, &wl, &thr, &res, &ray_o, &ray_d, &sh, &contrib, &hit, &aux, &counts, &ctrl}) b->leak(); for (DevBuf &b : stack_ovf) b.leak(); }
};

struct Workspace {
    StateBufs sb;
    // Single-pass renders repeated with the same shape (bench, animation frames) reuse the uploaded plan: the pass pixel
    // table (4 MB at 512^2), block tables and the regions' initial share of the samples.
    std::vector<uint64_t> plan_key;          // empty = nothing cached
    uint64_t plan_n_pix = 0;
    DevBuf counts_init; unsigned long long counts_total = 0; uint32_t counts_regions = 0;
    DevBuf block_buf, blocks, block_of, spiral, pix, pix_inv, rec_a, rec_b, film, bands;
    void *host_film = nullptr; size_t host_film_bytes = 0;       // pinned staging buffer of msk_gpu_render's film copy-back
    ~Workspace() { if (host_film) (void) hipHostFree(host_film); }
    uint32_t n_bands = 0;
    DevBuf aov_rec[MSK_MAX_AOV_GROUPS + 1], aov_block_buf[MSK_MAX_AOV_GROUPS + 1];   // [n_groups] = the nested path's RGB
    DevBuf direct_counters, direct_ovf;      // the "direct" integrator's counters and stack overflow (run_direct)
};

// what msk_gpu_render_aov asked for, in record groups of three channels (see AovParams)
struct AovPlan {
    uint32_t n_channels = 0;                 // film channels after X,Y,Z,A,W
    uint32_t n_groups = 0;                   // primary-hit groups
    uint32_t code[MSK_MAX_AOV_GROUPS] = {};
    int32_t out_ch[MSK_MAX_AOV_GROUPS + 1][5];   // film channel of each block channel, -1 = unused
    bool rgba = false;                       // group n_groups: nested path integrator R,G,B (+ A = the weight sum)
};

struct EventPool {
    msk_ctx *ctx; size_t next = 0; std::vector<hipEvent_t> *pool = nullptr;       // pool: ctx->events unless told otherwise
    // nullptr when the runtime cannot create another event: the dispatch then simply carries no timestamps
    // (hipExtLaunchKernelGGL takes null events) and the statistics miss that launch; nothing else depends on events
    hipEvent_t get() {
        std::vector<hipEvent_t> &v = pool ? *pool : ctx->events;
        while (next >= v.size()) {
            hipEvent_t e = nullptr;
            if (hipEventCreate(&e) != hipSuccess || !e) { (void) hipGetLastError(); return nullptr; }
            v.push_back(e);
        }
        return v[next++];
    }
};

void free_workspace(msk_scene *scene) { delete scene->ws; scene->ws = nullptr; }

static void sum_events(std::vector<std::pair<hipEvent_t, hipEvent_t>> &v, float *ms) {
    for (auto &p : v) { float t = 0; if (p.first && p.second && hipEventElapsedTime(&t, p.first, p.second) == hipSuccess) *ms += t; }
}

// Every wait of a render for its device outside the wavefront loop (which has wait_any): the wait mode of MSK_WAIT and the wall
// limit of MSK_WATCHDOG_S x `limit_scale` (the loop's limit is per sync group — a few milliseconds of work; MSK_RNG_PCG_BLOCK
// renders in ONE kernel that legitimately runs for as long as the job takes, and passes 30: an hour at the default).  A wait
// that runs out loses the context exactly as one inside the loop does.  Calling thread only.
static int ctx_sync(msk_ctx *ctx, hipStream_t stream, const char *what, double limit_scale) {
    mskwd::Limits lim = mskwd::limits_from_env();
    lim.wall_s *= limit_scale;
    const mskwd::Progress p(lim);
    const mskwd::Waiter w{mskwd::wait_mode_from_env(), ctx->hub};
    mskwd::Ticket t;
    t.stream = stream; t.slot = 0; t.event = ctx->wait_events[0];
    HIP_TRY(ctx, mskwd::arm(w, t));
    mskwd::Ticket *tp = &t;
    hipError_t es = hipSuccess;
    if (mskwd::wait_any(w, &tp, 1, p, &es) < 0) {
        ctx->lost = true;
        return fail(ctx, MSK_ERR_HIP, "no progress: %s did not finish within %g s (MSK_WATCHDOG_S); the context is lost", what, lim.wall_s);
    }
    HIP_TRY(ctx, es);
    return MSK_OK;
}

// ------------------------------------------------------------------------------------------
// kernel dispatch: WHAT runs is decided in msk_plan.h (LaunchPlan); each function here picks the instantiation the plan names
// and launches it, nothing else.
// t0 / t1: events that take the kernel's own start / end timestamps (hipExtLaunchKernelGGL: no extra packets in the queue,
// unlike hipEventRecord, which cost 2 % of a bench step at three records per iteration), or nullptr
// ------------------------------------------------------------------------------------------
// f(std::integral_constant<int, M>{}) with M = mode: the one place where a trace mode becomes a template argument
template <typename F> static void with_trace_mode(int mode, F &&f) {
    switch (mode) {
    case 0: f(std::integral_constant<int, 0>{}); break;
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 4: f(std::integral_constant<int, 4>{}); break;
    case 5: f(std::integral_constant<int, 5>{}); break;
    case 6: f(std::integral_constant<int, 6>{}); break;
    default: f(std::integral_constant<int, 3>{}); break;
    }
}

static void launch_trace(const msk_scene *sc, const mskplan::LaunchPlan &plan, hipStream_t stream, const PathState &st, const PassParams &pp,
                         hipEvent_t t0 = nullptr, hipEvent_t t1 = nullptr) {
    const dim3 grid((pp.region_count * plan.trace_waves * MSK_WAVE + MSK_BLOCK - 1) / MSK_BLOCK), block(MSK_BLOCK);
    const size_t lds = plan.trace_lds_bytes;
    if (plan.trace_family == mskplan::TRACE_FAMILY_Q) {
        hipExtLaunchKernelGGL(k_trace_q, grid, block, lds, stream, t0, t1, 0, sc->dev, st, pp, plan.queue_refill, (uint32_t) (plan.bits_off / 16));
        return;
    }
    with_trace_mode(plan.trace_mode, [&](auto m) {
        constexpr int M = decltype(m)::value;
        if (plan.trace_family == mskplan::TRACE_FAMILY_PLAIN) hipExtLaunchKernelGGL(k_trace<M>, grid, block, lds, stream, t0, t1, 0, sc->dev, st, pp);
        else if constexpr (M != mskplan::TRACE_WIDE4_LDS)         // (the tree in LDS is never walked with lane replacement: no k_trace_r<3>)
            hipExtLaunchKernelGGL(k_trace_r<M>, grid, block, lds, stream, t0, t1, 0, sc->dev, st, pp, plan.refill, plan.max_inner);
    });
}

template <bool LDS_TABLES>
static void launch_shade_t(const msk_scene *sc, const mskplan::LaunchPlan &plan, dim3 grid, hipStream_t stream, const PathState &st, const PassParams &pp,
                           hipEvent_t t0, hipEvent_t t1) {
#define MSK_SHADE(...) hipExtLaunchKernelGGL((__VA_ARGS__), grid, dim3(MSK_BLOCK), plan.shade_lds_bytes, stream, t0, t1, 0, sc->dev, st, pp)
    // (the families' cases come from the list, msk_kernels.h; no default: -Wswitch names a kind that has no case)
#define MSK_CASE(S, TABLES, KIND, SHADE, SERIAL) case mskplan::KIND: MSK_SHADE(k_shade_gen_##S<LDS_TABLES>); break;
    switch (plan.shade_kind) {
    case mskplan::SHADE_DIFFUSE: MSK_SHADE(k_shade_gen<LDS_TABLES, true>); break;
    case mskplan::SHADE_REGULAR: MSK_SHADE(k_shade_gen<LDS_TABLES, false, true>); break;
    case mskplan::SHADE_GENERAL: MSK_SHADE(k_shade_gen<LDS_TABLES, false>); break;
    MSK_FAMILIES(MSK_CASE)
    }
#undef MSK_CASE
#undef MSK_SHADE
}
static void launch_shade(const msk_scene *sc, const mskplan::LaunchPlan &plan, dim3 grid, hipStream_t stream, const PathState &st, const PassParams &pp,
                         hipEvent_t t0, hipEvent_t t1) {
    if (plan.lds_tables) launch_shade_t<true>(sc, plan, grid, stream, st, pp, t0, t1);
    else launch_shade_t<false>(sc, plan, grid, stream, st, pp, t0, t1);
}

// the iteration loop on the device: one bounded launch = up to plan.fused_iters sweeps of every region
static void launch_fused(const msk_scene *sc, const mskplan::LaunchPlan &plan, dim3 grid, hipStream_t stream, const PathState &st, const PassParams &pp) {
#define MSK_FUSED(...) hipExtLaunchKernelGGL((__VA_ARGS__), grid, dim3(MSK_BLOCK), plan.fused_lds_bytes, stream, nullptr, nullptr, 0, sc->dev, st, pp, \
                                             plan.fused_iters, plan.fused_queue_f4, plan.fused_trace_f4)
#define MSK_CASE_H(S, TABLES, KIND, SHADE, SERIAL) case mskplan::KIND: MSK_FUSED(k_wavefront_h_##S); break;
#define MSK_CASE(S, TABLES, KIND, SHADE, SERIAL) case mskplan::KIND: MSK_FUSED(k_wavefront_##S); break;
    if (plan.fused_h) switch (plan.shade_kind) {      // the tree in HBM (trace mode 6)
    case mskplan::SHADE_DIFFUSE: MSK_FUSED(k_wavefront_h<true>); break;
    case mskplan::SHADE_REGULAR: MSK_FUSED(k_wavefront_h<false, true>); break;
    case mskplan::SHADE_GENERAL: MSK_FUSED(k_wavefront_h<false>); break;
    MSK_FAMILIES(MSK_CASE_H)
    }
    else switch (plan.shade_kind) {                   // everything in LDS (trace mode 0)
    case mskplan::SHADE_DIFFUSE: MSK_FUSED(k_wavefront<true>); break;
    case mskplan::SHADE_REGULAR: MSK_FUSED(k_wavefront<false, true>); break;
    case mskplan::SHADE_GENERAL: MSK_FUSED(k_wavefront<false>); break;
    MSK_FAMILIES(MSK_CASE)
    }
#undef MSK_CASE
#undef MSK_CASE_H
#undef MSK_FUSED
}

// ------------------------------------------------------------------------------------------
// the wavefront loop
// ------------------------------------------------------------------------------------------
namespace {

// what the parts of one run_wavefront call share
struct Wavefront {
    msk_scene *sc; StateBufs &sb; const mskplan::LaunchPlan &plan; const mskplan::RenderKnobs &knobs;
    const AovParams *aov;              // the record groups of an "aov" render (k_aov_primary after every sweep), or nullptr
    uint32_t region_size;
    bool timing;                       // the caller asked for msk_stats
    // A timed dispatch costs ~6 us more than an untimed one (completion signal + timestamps): 2 % of a bench step when every
    // launch is timed.  MSK_TIMING_EVERY=n times the launches of every n-th sync group only (rotating from render to render so
    // that repeated renders cover all groups); msk_stats::ms_trace / ms_shade / n_*_launches then describe that sample.
    uint32_t phase;
    mskwd::Waiter waiter;
};

// One part of the pool: the regions [first, first + count) and their wavefront loop on one stream.  The parts' loops run at the
// same time: regions are independent — each owns its slots, its share of the samples and its counters — and a shading
// launch of one part fills the gaps of a traversal launch of another (and the other way round), which one launch at a time
// leaves open at its start, its end and wherever its waves wait.  Measured with two concurrent half-size renders before
// this was built: 49.3 against 55.0 ms for the bench step.  WHO drives the loops is a separate choice (MSK_HOST_THREADS below).
struct Part {
    const Wavefront *wf = nullptr;
    uint32_t first = 0, count = 0; hipStream_t stream = nullptr; Ctrl *d_ctrl = nullptr, *h_ctrl = nullptr; EventPool ev{nullptr};
    msk_stats st; int rc = MSK_OK; unsigned long long expected = 0, culled = 0; std::string err; bool lost = false;
    // the loop's state between two sync groups
    PassParams pp; uint32_t grid = 0, it = 0, gi = 0, parity = 0, last_iters = 0; bool fused_now = false, done = false; size_t ev_mark = 0;
    // Two alternating sets of events: a group's timestamps are read (hipEventElapsedTime is a host call of a few
    // microseconds, 32 of them per group) after the NEXT group has been queued, not while the GPU waits for work.
    std::vector<std::pair<hipEvent_t, hipEvent_t>> cur_shade, cur_trace, pend_shade, pend_trace;
    mskwd::Progress watchdog;                          // msk_watchdog.h: a wall limit per sync group + "the counters stand still"
    mskwd::Ticket ticket;
    explicit Part(const mskwd::Limits &l) : watchdog(l) { std::memset(&st, 0, sizeof st); }

    void read_pending();
    int queue_group();
    int finish_group();
};

void Part::read_pending() {
    if (!wf->timing) return;
    sum_events(pend_shade, &st.ms_shade); sum_events(pend_trace, &st.ms_trace);
    st.n_shade_launches += (uint32_t) pend_shade.size(); st.n_trace_launches += (uint32_t) pend_trace.size();
    pend_shade.clear(); pend_trace.clear();
}

// MSK_DUMP_RAYS=<file> (+ MSK_DUMP_ITER, default 12; MSK_DUMP_STRIDE, default 32), measurements only: the rays the traversal
// launch of that iteration is about to walk — every MSK_DUMP_STRIDE-th region of the first part, its live slots in the
// order the kernel takes them (shadow-carrying slots first) — written to the file for the host-side scheduler model
// (tools/micro/sched_model.cpp).  Header {'MSKR', regions, region_size, stride}; per region {count, ns}, then count x
// {ray_o, ray_d (w = tmax as the kernel reads it), sh} float4.
static void dump_rays(const Part &p) {
    const StateBufs &sb = p.wf->sb;
    const uint32_t region_size = p.wf->region_size, dump_stride = p.wf->knobs.dump_stride;
    if (hipStreamSynchronize(p.stream) != hipSuccess) return;
    std::vector<RegionCtl> ctl(p.count);
    if (hipMemcpy(ctl.data(), sb.counts.as<RegionCtl>() + p.first, p.count * sizeof(RegionCtl), hipMemcpyDeviceToHost) != hipSuccess) return;
    FILE *f = std::fopen(p.wf->knobs.dump_rays, "wb");
    if (!f) return;
    const uint32_t n_dump = (p.count + dump_stride - 1) / dump_stride;
    const uint32_t head[4] = {0x524b534du, n_dump, region_size, dump_stride};
    std::fwrite(head, 4, 4, f);
    std::vector<float4> ho(2 * (size_t) region_size), hd(2 * (size_t) region_size), hs(2 * (size_t) region_size);
    for (uint32_t r = 0; r < p.count; r += dump_stride) {
        const size_t base = (size_t) (p.first + r) * 2 * region_size;
        (void) hipMemcpy(ho.data(), sb.st.ray_o + base, ho.size() * 16, hipMemcpyDeviceToHost);
        (void) hipMemcpy(hd.data(), sb.st.ray_d + base, hd.size() * 16, hipMemcpyDeviceToHost);
        (void) hipMemcpy(hs.data(), sb.st.sh + base, hs.size() * 16, hipMemcpyDeviceToHost);
        const uint32_t count = ctl[r].count, ns = ctl[r].half_ns >> 1, half = ctl[r].half_ns & 1u;
        const uint32_t cn[2] = {count, ns};
        std::fwrite(cn, 4, 2, f);
        for (uint32_t c = 0; c < count; ++c) {
            const size_t slot = (size_t) half * region_size + (c < ns ? c : region_size - 1 - (c - ns));
            float4 rec[3] = {ho[slot], hd[slot], c < ns ? hs[slot] : make_float4(0, 0, 0, 0)};
            if (std::signbit(rec[1].w)) rec[1].w = INFINITY;          // slot_tmax: a bounce ray keeps -pdf there
            std::fwrite(rec, 16, 3, f);
        }
    }
    std::fclose(f);
}

// queues one sync group of the part's loop: `sync_group` iterations (or one k_wavefront launch), the counters' reduction and
// their copy to the host, and whatever the wait mode needs behind them
int Part::queue_group() {
    const Wavefront &w = *wf;
    const mskplan::LaunchPlan &plan = w.plan;
    ev.next = ev_mark + (size_t) parity * 4 * plan.sync_group;
    const bool timed = w.timing && (gi + w.phase) % plan.timing_every == 0;
    if (fused_now) {
        // (not timed: msk_stats::ms_shade / ms_trace stay the sums of k_shade_gen / k_trace launches)
        launch_fused(w.sc, plan, dim3(grid), stream, w.sb.st, pp);
        it += plan.fused_iters; last_iters = plan.fused_iters;
        st.launches_wavefront += 1;
    } else {
        for (uint32_t g = 0; g < plan.sync_group; ++g, ++it) {
            hipEvent_t a = nullptr, b = nullptr, c = nullptr, d = nullptr;
            if (timed) { a = ev.get(); b = ev.get(); c = ev.get(); d = ev.get(); }
            const bool have_ev = a && b && c && d;
            launch_shade(w.sc, plan, dim3(grid), stream, w.sb.st, pp, a, b);
            if (w.knobs.dump_rays && it == w.knobs.dump_iter && first == 0) dump_rays(*this);      // (measurements only: MSK_DUMP_RAYS)
            launch_trace(w.sc, plan, stream, w.sb.st, pp, c, d);
            st.launches_shade += 1; st.launches_trace += 1;
            if (w.aov && w.aov->n_groups) hipLaunchKernelGGL(k_aov_primary, dim3(grid), dim3(MSK_BLOCK), 0, stream, w.sc->dev, w.sb.st, pp, *w.aov);
            if (timed && have_ev) { cur_shade.push_back({a, b}); cur_trace.push_back({c, d}); }
        }
        last_iters = plan.sync_group;
    }
    read_pending();                    // the previous group's, while this one runs
    HIP_TRY_SLOT(&err, hipMemsetAsync(d_ctrl, 0, sizeof(Ctrl), stream));
    hipLaunchKernelGGL(k_reduce_ctl, dim3(std::min(64u, (count + MSK_BLOCK - 1) / MSK_BLOCK)), dim3(MSK_BLOCK), 0, stream,
                       w.sb.counts.as<RegionCtl>() + first, count, d_ctrl);
    HIP_TRY_SLOT(&err, hipGetLastError());
    HIP_TRY_SLOT(&err, hipMemcpyAsync(h_ctrl, d_ctrl, sizeof(Ctrl), hipMemcpyDeviceToHost, stream));
    HIP_TRY_SLOT(&err, mskwd::arm(w.waiter, ticket));
    return MSK_OK;
}

// after the group's last command has completed: is the part done, stalled, or ready for its thin end?
int Part::finish_group() {
    const mskplan::LaunchPlan &plan = wf->plan;
    pend_shade.swap(cur_shade); pend_trace.swap(cur_trace); cur_shade.clear(); cur_trace.clear(); parity ^= 1u; ++gi;
    const Ctrl &h = *h_ctrl;
    if (h.remaining == 0 && h.live == 0) {
        read_pending();
        ev.next = ev_mark;                              // every timestamp has been read: the events are free again
        st.samples = h.samples_done; st.segments = h.segments; st.shadow_rays = h.shadow_rays;
        st.invalid_samples = h.invalid;
        culled = h.culled;
        st.iterations = it;
        done = true;
        if (h.samples_done != expected)
            return fail_to(&err, MSK_ERR_HIP, "internal error: %llu of %llu samples finished", h.samples_done, expected);
        return MSK_OK;
    }
    if (watchdog.group_done(mskwd::Counters{h.samples_done, h.segments, h.remaining, h.live}) == mskwd::STALLED) {
        lost = true;
        return fail_to(&err, MSK_ERR_HIP, "no progress: %u sync groups of the wavefront loop changed nothing (%llu samples finished, %llu live paths, "
                       "%llu samples not started; MSK_WATCHDOG_GROUPS); the context is lost", watchdog.stalled(), h.samples_done, h.live, h.remaining);
    }
    if (plan.fused_ok && !fused_now && h.remaining == 0 && h.live * 100ull < (unsigned long long) plan.fused_tail_pct * count * wf->region_size)
        fused_now = true;                         // the thinning end of the pass: no more launches and host round trips per sweep
    if (it > 100000000u) return fail_to(&err, MSK_ERR_HIP, "wavefront loop did not terminate");
    return MSK_OK;
}

}  // namespace

// One host thread drives n of the parts: queues a group on each, then serves whichever finishes (wait_any), oldest first.
static void drive(int device, const mskwd::Waiter &waiter, Part *const *mine, int n) {
    (void) hipSetDevice(device);                    // the current device is per host thread
    Part *active[MSK_MAX_STREAMS];
    int n_active = 0;
    for (int i = 0; i < n; ++i) {
        mine[i]->rc = mine[i]->queue_group();
        if (mine[i]->rc == MSK_OK) active[n_active++] = mine[i];
    }
    while (n_active) {
        mskwd::Ticket *tickets[MSK_MAX_STREAMS];
        for (int i = 0; i < n_active; ++i) tickets[i] = &active[i]->ticket;
        hipError_t es = hipSuccess;
        const int hit = mskwd::wait_any(waiter, tickets, n_active, active[0]->watchdog, &es);
        if (hit < 0) {                              // the wall limit: nothing this thread waits for will be waited for again
            for (int i = 0; i < n_active; ++i) {
                Part &q = *active[i];
                q.lost = true;
                q.rc = fail_to(&q.err, MSK_ERR_HIP, "no progress: a sync group of the wavefront loop (iterations %u..%u, regions %u..%u) did not finish within "
                               "%g s (MSK_WATCHDOG_S); the context is lost", q.it - q.last_iters, q.it, q.first, q.first + q.count, q.watchdog.limits().wall_s);
            }
            return;
        }
        Part &p = *active[hit];
        for (int i = hit; i + 1 < n_active; ++i) active[i] = active[i + 1];
        --n_active;
        if (es != hipSuccess) { p.rc = fail_to(&p.err, MSK_ERR_HIP, "the wavefront loop's stream reported: %s", hipGetErrorString(es)); continue; }
        p.rc = p.finish_group();
        if (p.lost) return;                         // (stalled: the context is done, the other parts are not driven further)
        if (p.rc == MSK_OK && !p.done) {
            p.rc = p.queue_group();
            if (p.rc == MSK_OK) active[n_active++] = &p;
        }
    }
}

// The regions' records at the start of a pass: each region's share of the samples (mskplan::region_share).  The initial records
// are kept on the device and copied from there when the next render has the same shape.
static int reset_regions(msk_scene *sc, hipStream_t stream, StateBufs &sb, unsigned long long total, uint32_t n_regions) {
    msk_ctx *ctx = sc->ctx;
    Workspace *wsp = sc->ws;
    if (!(wsp && wsp->counts_total == total && wsp->counts_regions == n_regions && wsp->counts_init.p)) {
        std::vector<RegionCtl> init(n_regions);
        std::memset(init.data(), 0, init.size() * sizeof(RegionCtl));
        for (uint32_t r = 0; r < n_regions; ++r) { init[r].next_sample = 0; init[r].end_sample = mskplan::region_share(total, n_regions, r); }
        if (wsp) {
            HIP_TRY(ctx, wsp->counts_init.reserve(init.size() * sizeof(RegionCtl)));
            HIP_TRY(ctx, hipMemcpy(wsp->counts_init.p, init.data(), init.size() * sizeof(RegionCtl), hipMemcpyHostToDevice));
            wsp->counts_total = total; wsp->counts_regions = n_regions;
        } else {
            HIP_TRY(ctx, hipMemcpyAsync(sb.counts.p, init.data(), init.size() * sizeof(RegionCtl), hipMemcpyHostToDevice, stream));
            if (int rc = ctx_sync(ctx, stream, "the upload of the regions' records")) return rc;
        }
    }
    if (wsp) HIP_TRY(ctx, hipMemcpyAsync(sb.counts.p, wsp->counts_init.p, (size_t) n_regions * sizeof(RegionCtl), hipMemcpyDeviceToDevice, stream));
    return MSK_OK;
}

// ABI v7: the bytes of SoA path state this pass's launches were asked to move (counted from what the kernels
// read and write per live slot, not measured): a segment = a slot that is live after a shading sweep.
//   shading  176 B/segment (id 8, wl, thr, res, ray_d, hit in; id 8, wl, thr, res, ray_o, ray_d out; + aux 8 in / 8 out in the
//            general variant) - 64 B/sample (a new sample's thr = 1 and res = 0 are neither written nor read)
//            + 48 B/shadow ray (contrib in; sh, contrib out) + 20 B/sample (its record)
//   traversal 48 B/segment (ray_o, ray_d in; hit out) + per shadow ray: sh in, and ray_o again where the shadow rays are a
//            second queue of the launch (k_trace_q / k_trace: 32 B; k_trace_r walks both rays of a slot together: 16 B —
//            LaunchPlan::lane_refill, which leaves an LDS-resident scene forced onto k_trace_r<0> at 32 B)
//   a CULLED sample (round 9; counted in samples and in segments) moves its 20-byte record and nothing else: it never
//            holds a slot — 112 B less of shading (176 - 64; 128 with the general variant's aux) and 48 B less of traversal than the terms above give it
static void add_part_stats(msk_stats *stats, const Part &p, const mskplan::LaunchPlan &plan) {
    stats->samples += p.st.samples; stats->segments += p.st.segments; stats->shadow_rays += p.st.shadow_rays;
    stats->invalid_samples += p.st.invalid_samples;
    stats->iterations += p.st.iterations;
    stats->ms_trace += p.st.ms_trace; stats->ms_shade += p.st.ms_shade;
    stats->n_trace_launches += p.st.n_trace_launches; stats->n_shade_launches += p.st.n_shade_launches;
    stats->launches_trace += p.st.launches_trace; stats->launches_shade += p.st.launches_shade; stats->launches_wavefront += p.st.launches_wavefront;
    const unsigned long long seg = p.st.segments, smp = p.st.samples, shd = p.st.shadow_rays, cul = p.culled;
    const unsigned long long aux = plan.diffuse_only ? 0ull : 16ull;
    stats->bytes_shade += seg * (176ull + aux) + shd * 48ull + smp * 20ull - std::min(smp * 64ull, seg * 176ull) - cul * (112ull + aux);
    stats->bytes_trace += seg * 48ull + shd * (plan.lane_refill ? 16ull : 32ull) - cul * 48ull;
}

static PassParams pass_params(const msk_render_params *prm, uint32_t spp_owned, const uint4 *d_pix, const uint32_t *d_pix_to_j, float4 *rec_a, float *rec_b,
                              StateBufs &sb, uint32_t region_size, uint32_t n_regions, const mskplan::LaunchPlan &plan,
                              const AovParams *aov, float4 *aov_rgb, bool packed) {
    PassParams pp;
    pp.seed = prm->seed; pp.spp_owned = spp_owned; pp.sample_first = prm->sample_first;
    pp.sample_stride = prm->sample_stride ? prm->sample_stride : 1;
    pp.rr_depth = prm->rr_depth; pp.max_depth = prm->max_depth; pp.hide_emitters = prm->hide_emitters;
    pp.pix_table = d_pix; pp.pix_to_j = d_pix_to_j; pp.rec_a = rec_a; pp.rec_b = rec_b;
    pp.region_size = region_size; pp.n_regions = n_regions; pp.regions = sb.counts.as<RegionCtl>();
    pp.region_first = 0; pp.region_count = n_regions;
    pp.trace_split = plan.trace_split;
    pp.aov_rgb = aov_rgb;
    pp.aov_groups = aov ? aov->n_groups : 0u;
    for (uint32_t g = 0; g < MSK_MAX_AOV_GROUPS; ++g) pp.aov_rec[g] = aov && g < aov->n_groups ? aov->rec[g] : nullptr;
    pp.packed = packed ? 1u : 0u;
    pp.stack_ovf = nullptr;
    pp.cull = plan.cull ? 1u : 0u;
    pp.sort_scratch = plan.sort_on ? 1u : 0u;
    return pp;
}

// Renders the samples of `pix` (pass pixel table, host) into records; leaves records on device.
static int run_wavefront(msk_scene *sc, hipStream_t stream, const msk_render_params *prm, const mskplan::RenderKnobs &knobs, uint32_t spp_owned,
                         const uint4 *d_pix, const uint32_t *d_pix_to_j, uint64_t n_pix, float4 *rec_a, float *rec_b, StateBufs &sb,
                         uint32_t region_size, uint32_t n_regions, msk_stats *stats, EventPool &ev,
                         const AovParams *aov = nullptr, float4 *aov_rgb = nullptr, bool packed = false) {
    msk_ctx *ctx = sc->ctx;
    const unsigned long long total = (unsigned long long) n_pix * spp_owned;
    if (int rc = reset_regions(sc, stream, sb, total, n_regions)) return rc;
    mskplan::CallFacts call;
    call.region_size = region_size; call.aov_groups = aov ? aov->n_groups : 0u; call.aov_rgb = aov_rgb != nullptr;
    const mskplan::LaunchPlan plan = mskplan::make_launch_plan(sc->facts, call, knobs);
    const PassParams pp0 = pass_params(prm, spp_owned, d_pix, d_pix_to_j, rec_a, rec_b, sb, region_size, n_regions, plan, aov, aov_rgb, packed);
    const Wavefront wf{sc, sb, plan, knobs, aov, region_size, stats != nullptr, ctx->timing_phase++, mskwd::Waiter{mskwd::wait_mode_from_env(), ctx->hub}};
    const mskwd::Limits wd_limits = mskwd::limits_from_env();

    // how many loops: 4 by default (DESIGN.md §6 has 1 / 2 / 3 / 4); one for small jobs and caller-supplied streams
    uint32_t n_parts = std::min<uint32_t>(MSK_MAX_STREAMS, std::max(1u, knobs.streams));
    if (n_regions < 1024 || stream != ctx->stream) n_parts = 1;
    const uint32_t ovf_words = sc->dev.stack_total > sc->dev.stack_entries ? sc->dev.stack_total - sc->dev.stack_entries : 0;
    const std::vector<uint32_t> cut = mskplan::part_ranges(n_regions, n_parts, knobs.stream_skew);
    std::vector<Part> parts;
    parts.reserve(n_parts);
    for (uint32_t k = 0; k < n_parts; ++k) {
        parts.emplace_back(wd_limits);
        Part &p = parts.back();
        p.wf = &wf;
        p.first = cut[k]; p.count = cut[k + 1] - cut[k]; p.stream = k ? ctx->more_streams[k - 1] : stream;
        p.d_ctrl = sb.ctrl.as<Ctrl>() + k; p.h_ctrl = ctx->h_ctrl + k;
        p.ev = k ? EventPool{ctx, 0, &ctx->more_events[k - 1]} : EventPool{ctx, ev.next, ev.pool};
        p.ev_mark = p.ev.next;
        for (uint32_t r = p.first; r < p.first + p.count; ++r) p.expected += mskplan::region_share(total, n_regions, r);
        p.pp = pp0; p.pp.region_first = p.first; p.pp.region_count = p.count;
        p.grid = (p.count * MSK_WAVE + MSK_BLOCK - 1) / MSK_BLOCK;
        p.fused_now = plan.fused_all;
        p.ticket.stream = p.stream; p.ticket.slot = (int) k; p.ticket.event = ctx->wait_events[k];
        if (ovf_words) {                                // LaneStack overflow: one word per lane per extra entry, per launch
            const size_t lanes = (size_t) p.grid * MSK_BLOCK;
            HIP_TRY(ctx, sb.stack_ovf[k].reserve((size_t) ovf_words * lanes * 4));
            p.pp.stack_ovf = sb.stack_ovf[k].as<uint32_t>();
        }
    }
    // Who drives the parts' loops (MSK_HOST_THREADS): ONE host thread for all of them by default since round 6 — it queues a
    // group on every stream and then serves whichever finishes; the device always holds the other streams' queued groups while
    // the host turns one around.  Rounds 2-5 used one thread per part (MSK_HOST_THREADS=4): three more threads per context,
    // spinning with the poll wait (DESIGN.md §7 has both under a CPU quota).
    const uint32_t n_threads = std::min(n_parts, std::max(1u, knobs.host_threads));
    if (n_parts > 1)       // the regions' records (queued above) before the other streams read them
        if (int rc = ctx_sync(ctx, stream, "the regions' initial records")) return rc;
    {
        std::vector<std::vector<Part *>> mine(n_threads);
        for (uint32_t k = 0; k < n_parts; ++k) mine[k % n_threads].push_back(&parts[k]);
        std::vector<std::thread> others;
        for (uint32_t j = 1; j < n_threads; ++j) others.emplace_back([&, j]() { drive(ctx->device, wf.waiter, mine[j].data(), (int) mine[j].size()); });
        drive(ctx->device, wf.waiter, mine[0].data(), (int) mine[0].size());
        for (auto &t : others) t.join();
    }
    for (auto &p : parts) if (p.lost) ctx->lost = true;                                // the watchdog gave up on a part: the context is done
    for (auto &p : parts) if (p.rc) return fail(ctx, p.rc, "%s", p.err.c_str());      // first failing part, after the join
    if (stats) for (const Part &p : parts) add_part_stats(stats, p, plan);
    return MSK_OK;
}

// The "direct" integrator's pass: the records of `pix` by k_direct (msk_direct.h), cut into launches of a bounded number of rays
// (mskplan::make_direct_plan); every few launches the host waits through the watchdog's timed wait.  Leaves records on the device.
static int run_direct(msk_scene *sc, hipStream_t stream, const msk_render_params *prm, const msk_direct_params *dp, uint32_t spp_owned,
                      const uint4 *d_pix, const uint32_t *d_pix_to_j, uint64_t n_pix, float4 *rec_a, float *rec_b, msk_stats *stats, bool packed) {
    msk_ctx *ctx = sc->ctx;
    const uint64_t total = n_pix * spp_owned;
    if (total == 0) return MSK_OK;
    const mskplan::DirectPlan plan = mskplan::make_direct_plan(sc->facts, sc->dev.stack_entries, sc->dev.stack_total, sc->bvh_depth,
                                                               dp->light_samples, dp->bsdf_samples, total);
    if (!sc->ws) sc->ws = new Workspace();
    Workspace &ws = *sc->ws;
    StateBufs none;                                      // no path state: the regions' pointer of PassParams stays null
    const PassParams pp = pass_params(prm, spp_owned, d_pix, d_pix_to_j, rec_a, rec_b, none, 0u, 0u, mskplan::LaunchPlan{}, nullptr, nullptr, packed);
    PathState st;
    std::memset(&st, 0, sizeof st);
    DeviceScene ds = sc->dev;
    ds.stack_entries = plan.stack_entries;
    const size_t counter_bytes = (size_t) MSK_DIRECT_COUNTER_LINES * 8 * sizeof(unsigned long long);
    HIP_TRY(ctx, ws.direct_counters.reserve(counter_bytes));
    HIP_TRY(ctx, hipMemsetAsync(ws.direct_counters.p, 0, counter_bytes, stream));
    const uint32_t grid_max = plan.grid_blocks(std::min<uint64_t>(total, plan.records_per_launch));
    if (plan.ovf_entries) HIP_TRY(ctx, ws.direct_ovf.reserve((size_t) plan.ovf_entries * grid_max * MSK_BLOCK * 4));
    DirectArgs da;
    da.n_light = dp->light_samples; da.n_bsdf = dp->bsdf_samples;
    da.per_wave = plan.records_per_wave; da.tables_mode = plan.tables_mode; da.stack_f4 = plan.stack_f4;
    da.stack_ovf = plan.ovf_entries ? ws.direct_ovf.as<uint32_t>() : nullptr;
    da.counters = ws.direct_counters.as<unsigned long long>();
    uint32_t n_launches = 0;
    for (uint64_t first = 0; first < total; first += plan.records_per_launch) {
        da.rec_first = first; da.rec_count = std::min<uint64_t>(plan.records_per_launch, total - first);
        const dim3 grid(plan.grid_blocks(da.rec_count)), block(MSK_BLOCK);
        if (sc->facts.has_lens) {              // the `thinlens` sensor: the instantiations whose camera ray starts on the lens
            if (plan.form == mskplan::TRACE_BIN_LDS) hipLaunchKernelGGL((k_direct<0, true>), grid, block, plan.lds_bytes, stream, ds, st, pp, da);
            else if (plan.form == mskplan::TRACE_WIDE4_HALF) hipLaunchKernelGGL((k_direct<6, true>), grid, block, plan.lds_bytes, stream, ds, st, pp, da);
            else hipLaunchKernelGGL((k_direct<1, true>), grid, block, plan.lds_bytes, stream, ds, st, pp, da);
        } else
        if (plan.form == mskplan::TRACE_BIN_LDS) hipLaunchKernelGGL(k_direct<0>, grid, block, plan.lds_bytes, stream, ds, st, pp, da);
        else if (plan.form == mskplan::TRACE_WIDE4_HALF) hipLaunchKernelGGL(k_direct<6>, grid, block, plan.lds_bytes, stream, ds, st, pp, da);
        else hipLaunchKernelGGL(k_direct<1>, grid, block, plan.lds_bytes, stream, ds, st, pp, da);
        HIP_TRY(ctx, hipGetLastError());
        // (a launch is bounded work — DirectPlan::records_per_launch — so a group of eight is what one timed wait covers)
        if (++n_launches % 8u == 0u)
            if (int rc = ctx_sync(ctx, stream, "a group of k_direct launches")) return rc;
    }
    std::vector<unsigned long long> h((size_t) MSK_DIRECT_COUNTER_LINES * 8, 0ull);
    HIP_TRY(ctx, hipMemcpyAsync(h.data(), ws.direct_counters.p, counter_bytes, hipMemcpyDeviceToHost, stream));
    if (int rc = ctx_sync(ctx, stream, "the last k_direct launches of a pass")) return rc;
    if (stats) {
        for (uint32_t l = 0; l < MSK_DIRECT_COUNTER_LINES; ++l) {
            stats->samples += h[l * 8]; stats->segments += h[l * 8 + 1]; stats->shadow_rays += h[l * 8 + 2]; stats->invalid_samples += h[l * 8 + 3];
        }
        stats->iterations += n_launches;
    }
    return MSK_OK;
}

// samples per pixel this call renders: s = sample_first + k * sample_stride < spp.  64-bit: spp - first + stride - 1 wraps in
// 32 bits (spp 0xFFFFFFFF, stride 4095 owns 1048833 samples; a 32-bit sum would give 0 and render nothing)
static unsigned long long owned_spp(const msk_render_params *p) {
    const unsigned long long ss = p->sample_stride ? p->sample_stride : 1;
    return p->sample_first < p->spp ? ((unsigned long long) p->spp - p->sample_first + ss - 1) / ss : 0;
}

static int check_params(msk_ctx *ctx, const msk_render_params *p, int block_min) {
    if (!p) return fail(ctx, MSK_ERR_INVALID_ARG, "render params are NULL");
    if (p->rng_mode != MSK_RNG_COUNTER && p->rng_mode != MSK_RNG_PCG_BLOCK)
        return fail(ctx, MSK_ERR_INVALID_ARG, "rng_mode %d is neither MSK_RNG_COUNTER nor MSK_RNG_PCG_BLOCK", p->rng_mode);
    if (p->spp == 0) return fail(ctx, MSK_ERR_INVALID_ARG, "spp must be > 0");
    // the path state holds the OWNED sample index (PathState::id: s_own | depth << 20); the RNG key takes the global one,
    // first + s_own * stride, in full 32 bits.  So the limit is on the samples this call owns, not on spp.  (MSK_RNG_PCG_BLOCK
    // cannot shard samples — below — so there the two are the same.)
    if (owned_spp(p) > (1ull << MSK_DEPTH_SHIFT))
        return fail(ctx, MSK_ERR_UNSUPPORTED, "spp %u, sample_first %u, sample_stride %u: %llu samples per pixel in this call, at most %u "
                    "(the path state holds 20 bits of sample index); shard the samples with sample_first / sample_stride",
                    p->spp, p->sample_first, p->sample_stride, owned_spp(p), 1u << MSK_DEPTH_SHIFT);
    if (p->rr_depth <= 0) return fail(ctx, MSK_ERR_INVALID_ARG, "\"rr_depth\" must be set to a value greater than zero!");
    if (p->max_depth < 0 && p->max_depth != -1)
        return fail(ctx, MSK_ERR_INVALID_ARG, "\"max_depth\" must be set to -1 (infinite) or a value >= 0");
    // the path state holds 12 bits of depth: a path is cut after bounce MSK_MAX_DEPTH.  Unreachable with Russian roulette from a
    // depth below that (survival <= 0.95 per bounce); a bound or a roulette start beyond it would be cut silently, so refuse
    if (p->max_depth > (int) MSK_MAX_DEPTH)
        return fail(ctx, MSK_ERR_UNSUPPORTED, "max_depth %d: the path state holds bounces up to %u", p->max_depth, MSK_MAX_DEPTH);
    if (p->max_depth < 0 && p->rr_depth > (int) MSK_MAX_DEPTH)
        return fail(ctx, MSK_ERR_UNSUPPORTED, "rr_depth %d with unbounded max_depth: the path state holds bounces up to %u", p->rr_depth, MSK_MAX_DEPTH);
    if (p->block_size < block_min || p->block_size > 4096)        // (a pixel's place in its block is two 16-bit fields: PassParams::pix_table)
        return fail(ctx, MSK_ERR_INVALID_ARG, "block_size %d outside [%d, 4096]", p->block_size, block_min);
    const uint32_t bs = p->block_stride ? p->block_stride : 1;
    if (p->block_first >= bs) return fail(ctx, MSK_ERR_INVALID_ARG, "shard selector out of range");
    // MSK_RNG_PCG_BLOCK: a block's samples draw from ONE sequential PCG32 stream (samplers/independent.cpp:9-35), and how far a
    // sample advances it is only known once its path has been traced: a shard of the sample indices would start the stream at
    // the same place as every other shard and draw the same numbers (n shards summed = n copies of one spp / n render).  The
    // blocks' streams are independent: this mode shards by blocks (block_first / block_stride) only.
    if (p->rng_mode == MSK_RNG_PCG_BLOCK && (p->sample_first != 0 || (p->sample_stride != 0 && p->sample_stride != 1)))
        return fail(ctx, MSK_ERR_UNSUPPORTED, "MSK_RNG_PCG_BLOCK: the samples of a block share one sequential PCG32 stream and cannot be sharded "
                    "(sample_first %u, sample_stride %u); shard the blocks with block_first / block_stride", p->sample_first, p->sample_stride);
    return MSK_OK;
}

// The blocks of the spiral schedule this call renders: every block_stride-th from block_first on, unless it owns no sample.  A block
// whose bordered area misses the crop window adds nothing to the film (accumulate_2d clips it to nothing, imageblock.cpp:133-150):
// it is not rendered.
struct OwnedBlocks {
    int nbx = 0, nby = 0;
    std::vector<int32_t> block_of;         // [by * nbx + bx] -> index into `owned`, -1 = not rendered by this call
    std::vector<uint32_t> spiral_id;       // [by * nbx + bx] -> place in the spiral order
    std::vector<BlockInfo> owned;
};
static OwnedBlocks owned_blocks(const msk_scene *sc, const msk_render_params *prm) {
    OwnedBlocks o;
    const DeviceScene &ds = sc->dev;
    const int border = ds.filter_border;
    const std::vector<HostBlock> all = spiral_blocks(ds.width, ds.height, prm->block_size, &o.nbx, &o.nby);
    const uint32_t bstride = prm->block_stride ? prm->block_stride : 1;
    const bool nothing = owned_spp(prm) == 0;
    o.block_of.assign((size_t) o.nbx * o.nby, -1);
    o.spiral_id.assign((size_t) o.nbx * o.nby, 0);
    for (size_t id = 0; id < all.size(); ++id) {
        const HostBlock &b = all[id];
        o.spiral_id[(size_t) b.by * o.nbx + b.bx] = (uint32_t) id;
        if (id % bstride != prm->block_first || nothing) continue;
        if (b.off_x - border >= ds.crop_x + ds.crop_w || b.off_x + b.size_x + border <= ds.crop_x ||
            b.off_y - border >= ds.crop_y + ds.crop_h || b.off_y + b.size_y + border <= ds.crop_y) continue;
        o.block_of[(size_t) b.by * o.nbx + b.bx] = (int32_t) o.owned.size();
        o.owned.push_back(BlockInfo{b.off_x, b.off_y, b.size_x, b.size_y, 0u, (uint32_t) o.owned.size()});
    }
    return o;
}


// MSK_RNG_PCG_BLOCK: the reference's sampler as written — one PCG32 stream per block, so one lane per block (msk_serial.h).
// Same block schedule, shards, crop window and Film::put as the wavefront path; a fidelity mode, not a fast one.
static int render_serial(msk_scene *sc, const msk_render_params *prm, float *d_film, hipStream_t stream, msk_stats *stats) {
    msk_ctx *ctx = sc->ctx;
    const int border = sc->dev.filter_border;
    EventPool ev{ctx, 0};
    hipEvent_t t_begin = ev.get(), t_end = ev.get();
    if (t_begin) (void) hipEventRecord(t_begin, stream);
    const int bs = prm->block_size;
    OwnedBlocks ob = owned_blocks(sc, prm);
    std::vector<BlockInfo> &owned = ob.owned;
    const uint32_t buf_stride = (uint32_t) ((bs + 2 * border) * (bs + 2 * border)) * 5;
    if (!sc->ws) sc->ws = new Workspace();
    Workspace &ws = *sc->ws;
    ws.plan_key.clear();                                 // the block tables below replace whatever plan a wavefront render cached
    const size_t buf_bytes = std::max<size_t>(owned.size(), 1) * buf_stride * 4;
    HIP_TRY(ctx, ws.block_buf.reserve(buf_bytes));
    HIP_TRY(ctx, ws.blocks.upload(owned)); HIP_TRY(ctx, ws.block_of.upload(ob.block_of)); HIP_TRY(ctx, ws.spiral.upload(ob.spiral_id));
    HIP_TRY(ctx, hipMemsetAsync(ws.block_buf.p, 0, buf_bytes, stream));
    DevBuf counters, ovf;
    HIP_TRY(ctx, counters.reserve(32));
    HIP_TRY(ctx, hipMemsetAsync(counters.p, 0, 32, stream));
    // few blocks (BASELINE config 1 has 64): one block per WAVE — the GPU holds ~2000 of this kernel's waves at once, and a wave that
    // runs one scalar loop does not pay for the branches of 63 others (config 1: 3.0 s -> see profiles/r04_pcg_block_config1.txt)
    const bool per_wave = owned.size() <= env_u32("MSK_SERIAL_PER_WAVE_MAX", 16384);
    const uint32_t grid = (uint32_t) ((owned.size() * (per_wave ? MSK_WAVE : 1) + MSK_BLOCK - 1) / MSK_BLOCK);
    // the binary tree's stack: depth + 2 entries, the first sc->dev.stack_entries of them in LDS
    DeviceScene ds = sc->dev;
    const uint32_t need = (uint32_t) sc->bvh_depth + 2u;
    if (ds.stack_entries > need) ds.stack_entries = (need + 3u) & ~3u;
    const uint32_t ovf_words = need > ds.stack_entries ? need - ds.stack_entries : 0u;
    if (ovf_words && grid) HIP_TRY(ctx, ovf.reserve((size_t) ovf_words * grid * MSK_BLOCK * 4));
    if (grid) {
        SerialParams sp;
        sp.seed = prm->seed; sp.spp = prm->spp; sp.sample_first = prm->sample_first; sp.sample_stride = prm->sample_stride;
        sp.rr_depth = prm->rr_depth; sp.max_depth = prm->max_depth; sp.hide_emitters = prm->hide_emitters;
        sp.blocks = ws.blocks.as<BlockInfo>(); sp.n_blocks = (uint32_t) owned.size();
        sp.block_buf = ws.block_buf.as<float>(); sp.buf_stride = buf_stride;
        sp.stack_ovf = ovf.as<uint32_t>(); sp.counters = counters.as<unsigned long long>(); sp.per_wave = per_wave ? 1u : 0u;
#define MSK_SERIAL(K) hipLaunchKernelGGL(K, dim3(grid), dim3(MSK_BLOCK), (size_t) ds.stack_entries * MSK_BLOCK * 4, stream, ds, sp)
#define MSK_LAUNCH_YES(S) MSK_SERIAL(k_path_serial_##S); break;
#define MSK_LAUNCH_NO(S) break;      /* (no such kernel, and not reached: render_impl refuses the call) */
#define MSK_CASE(S, TABLES, KIND, SHADE, SERIAL) case mskplan::KIND: MSK_LAUNCH_##SERIAL(S)
        switch (mskplan::shade_family(sc->facts)) {       // the scene's family (msk_plan.h), as the wavefront path's plan
        case mskplan::SHADE_DIFFUSE: case mskplan::SHADE_REGULAR: case mskplan::SHADE_GENERAL: MSK_SERIAL(k_path_serial); break;
        MSK_FAMILIES(MSK_CASE)
        }
#undef MSK_CASE
#undef MSK_LAUNCH_NO
#undef MSK_LAUNCH_YES
#undef MSK_SERIAL
    }
    FilmOut fo;
    fo.film = d_film; fo.stride = 5;
    for (int c = 0; c < 5; ++c) fo.ch[c] = c;
    hipLaunchKernelGGL(k_film_put, dim3((uint32_t) (((size_t) sc->dev.crop_w * sc->dev.crop_h + MSK_BLOCK - 1) / MSK_BLOCK)), dim3(MSK_BLOCK), 0, stream,
                       sc->dev, ws.blocks.as<BlockInfo>(), ws.block_of.as<int32_t>(), ws.spiral.as<uint32_t>(), ob.nbx, ob.nby, bs,
                       ws.block_buf.as<float>(), buf_stride, fo);
    if (t_end) (void) hipEventRecord(t_end, stream);
    HIP_TRY(ctx, hipGetLastError());
    unsigned long long h[4] = {0, 0, 0, 0};
    HIP_TRY(ctx, hipMemcpyAsync(h, counters.p, 32, hipMemcpyDeviceToHost, stream));
    // (one kernel for the whole job: the wall limit is 30 x MSK_WATCHDOG_S, an hour at the default)
    if (int rcw = ctx_sync(ctx, stream, "the MSK_RNG_PCG_BLOCK render (k_path_serial + Film::put)", 30.0)) { counters.leak(); ovf.leak(); return rcw; }
    if (stats) {
        stats->samples = h[0]; stats->segments = h[1]; stats->shadow_rays = h[2]; stats->invalid_samples = h[3]; stats->passes = 1;
        if (t_begin && t_end) (void) hipEventElapsedTime(&stats->ms_total, t_begin, t_end);
    }
    return MSK_OK;
}

static int render_impl(msk_scene *sc, const msk_render_params *prm, float *d_film, hipStream_t user_stream, msk_stats *stats,
                       const AovPlan *aov = nullptr, const msk_direct_params *direct = nullptr) {
    msk_ctx *ctx = sc->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int border = sc->dev.filter_border;
    int rc = check_params(ctx, prm, std::max(4, 2 * border));
    if (rc) return rc;
    if (prm->rng_mode == MSK_RNG_PCG_BLOCK) {
        if (direct) return fail(ctx, MSK_ERR_UNSUPPORTED, "MSK_RNG_PCG_BLOCK is not supported by the \"direct\" integrator (it uses MSK_RNG_COUNTER)");
        if (aov) return fail(ctx, MSK_ERR_UNSUPPORTED, "MSK_RNG_PCG_BLOCK renders the \"path\" integrator only (the \"aov\" integrator uses MSK_RNG_COUNTER)");
        if (sc->facts.has_lens)
            return fail(ctx, MSK_ERR_UNSUPPORTED, "MSK_RNG_PCG_BLOCK does not render a scene with a `thinlens` sensor (the reference's sampler draws no aperture "
                        "sample; use MSK_RNG_COUNTER)");
        if (stats) std::memset(stats, 0, sizeof *stats);
        return render_serial(sc, prm, d_film, user_stream ? user_stream : ctx->stream, stats);
    }
    hipStream_t stream = user_stream ? user_stream : ctx->stream;
    if (stats) std::memset(stats, 0, sizeof *stats);
    EventPool ev{ctx, 0};
    hipEvent_t t_begin = ev.get(), t_end = ev.get();
    if (t_begin) (void) hipEventRecord(t_begin, stream);
    const int W = sc->dev.width, H = sc->dev.height, bs = prm->block_size;
    OwnedBlocks ob = owned_blocks(sc, prm);
    std::vector<BlockInfo> &owned = ob.owned;
    const uint32_t bstride = prm->block_stride ? prm->block_stride : 1;
    const uint32_t spp_owned = (uint32_t) owned_spp(prm);            // <= 2^20 (check_params)
    const uint32_t per_block = (uint32_t) ((bs + 2 * border) * (bs + 2 * border));
    const uint32_t buf_stride = per_block * 5;
    if (!sc->ws) sc->ws = new Workspace();
    Workspace &ws = *sc->ws;
    DevBuf &d_block_buf = ws.block_buf, &d_blocks = ws.blocks, &d_block_of = ws.block_of, &d_spiral = ws.spiral;
    HIP_TRY(ctx, d_block_buf.reserve(std::max<size_t>(owned.size(), 1) * buf_stride * 4));
    const uint32_t n_aov_bufs = aov ? aov->n_groups + (aov->rgba ? 1u : 0u) : 0u;
    for (uint32_t g = 0; g < n_aov_bufs; ++g) {
        const uint32_t slot = g < aov->n_groups ? g : MSK_MAX_AOV_GROUPS;
        HIP_TRY(ctx, ws.aov_block_buf[slot].reserve(std::max<size_t>(owned.size(), 1) * buf_stride * 4));
    }
    const size_t rec_bytes = 20 + 16 * (size_t) n_aov_bufs;      // per sample
    // ---- plan passes: consecutive owned blocks whose records fit the budget
    size_t free_b = 0, total_b = 0;
    HIP_TRY(ctx, hipMemGetInfo(&free_b, &total_b));
    const mskplan::RenderKnobs knobs = mskplan::read_render_knobs();      // once per render: every pass runs under the same knobs
    uint32_t region_size, n_regions;
    uint64_t all_samples = 0;
    for (auto &b : owned) all_samples += (uint64_t) b.size_x * b.size_y * spp_owned;
    mskplan::pool_shape(sc->facts.trace_mode, all_samples, knobs, &region_size, &n_regions);
    const size_t n_slots = (size_t) region_size * n_regions;
    const size_t state_bytes = 2 * n_slots * 144 + 4096;                              // two halves per region (StateBufs::alloc)
    const size_t held = ws.rec_a.bytes + ws.rec_b.bytes + ws.sb.id.bytes * 144 / 8;     // reusable: counts as free
    free_b += held;
    free_b /= std::max(1u, ctx->device_sharers);
    size_t budget = getenv("MSK_RECORD_BUDGET_MB") ? (size_t) atoll(getenv("MSK_RECORD_BUDGET_MB")) << 20
                                                   : (free_b > state_bytes ? (size_t) ((free_b - state_bytes) * 0.8) : 0);
    const size_t rec_bytes_per_block_max = (size_t) bs * bs * spp_owned * rec_bytes;
    if (!owned.empty() && budget < rec_bytes_per_block_max)
        return fail(ctx, MSK_ERR_OOM, "not enough HBM for one block of sample records (%zu B needed, %zu B budget)",
                    rec_bytes_per_block_max, budget);
    std::vector<std::pair<size_t, size_t>> passes;   // [b0, b1) over `owned`
    for (size_t b0 = 0; b0 < owned.size();) {
        size_t b1 = b0, bytes = 0; uint32_t pixel_base = 0;
        while (b1 < owned.size()) {
            const size_t add = (size_t) owned[b1].size_x * owned[b1].size_y * spp_owned * rec_bytes;
            if (b1 > b0 && bytes + add > budget) break;
            owned[b1].pixel_base = pixel_base; pixel_base += (uint32_t) (owned[b1].size_x * owned[b1].size_y);
            bytes += add; ++b1;
        }
        passes.push_back({b0, b1}); b0 = b1;
    }
    // Default filter (border 2, footprint of five pixels) and blocks whose bordered width fits 12 lane columns: the records carry
    // their filter weights and the replay is k_resolve_rows.  Anything else: positions + k_resolve_blocks.
    // source rows per band of k_resolve_rows: 8 cuts a 32-pixel block's 36 target rows into 8 + 7 x 4, eight equal chains per block
    // (and 2048 waves for the 512^2 bench = two per SIMD, what the kernel's registers allow): 3.03 vs 3.35 ms with 10
    const uint32_t band_rounds = std::max(5u, env_u32("MSK_RESOLVE_ROUNDS", 8));
    const bool packed = border == 2 && (int) std::floor(sc->dev.filter_radius + 0.5f) == 2 && bs + 2 * border <= 3 * MSK_RR_COLS &&
                        !env_u32("MSK_RESOLVE_GENERIC", 0);
    const std::vector<uint64_t> plan_key = {(uint64_t) W, (uint64_t) H, (uint64_t) bs, (uint64_t) border, prm->block_first, bstride,
                                            spp_owned, passes.size(), owned.size(), (uint64_t) packed, band_rounds};
    const bool plan_cached = passes.size() == 1 && ws.plan_key == plan_key;
    if (!plan_cached) {
        ws.plan_key.clear();
        HIP_TRY(ctx, d_blocks.upload(owned)); HIP_TRY(ctx, d_block_of.upload(ob.block_of)); HIP_TRY(ctx, d_spiral.upload(ob.spiral_id));
    }
    StateBufs &sb = ws.sb;
    if (!owned.empty() && !direct) HIP_TRY(ctx, sb.alloc(n_slots, n_regions));      // (the "direct" integrator keeps no path state)
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_resolve;
    DevBuf &d_pix = ws.pix, &d_rec_a = ws.rec_a, &d_rec_b = ws.rec_b;
    for (auto &ps : passes) {
        uint64_t n_pix = ws.plan_n_pix;
        if (!plan_cached) {
            std::vector<uint4> pix;
            for (size_t b = ps.first; b < ps.second; ++b) {
                for (int y = 0; y < owned[b].size_y; ++y)
                    for (int x = 0; x < owned[b].size_x; ++x)       // PassParams::pix_table; the record of (pixel j, sample) is j * spp + sample
                        pix.push_back(make_uint4((uint32_t) ((owned[b].off_y + y) * W + owned[b].off_x + x), (uint32_t) x | ((uint32_t) y << 16),
                                                 (uint32_t) (owned[b].off_x - border), (uint32_t) (owned[b].off_y - border)));
            }
            HIP_TRY(ctx, d_pix.upload(pix));
            std::vector<uint32_t> inv((size_t) W * H, 0xffffffffu);       // film index -> pass pixel (PassParams::pix_to_j)
            for (size_t j = 0; j < pix.size(); ++j) inv[pix[j].x] = (uint32_t) j;
            HIP_TRY(ctx, ws.pix_inv.upload(inv));
            n_pix = pix.size();
            // k_resolve_rows work list: per block, bands of target rows that each cost at most `band_rounds` source rows
            // (the first band has no rows above it to wait for and the last one none below, so they take more target rows)
            std::vector<RowBand> bands;
            for (size_t b = ps.first; packed && b < ps.second; ++b) {
                const uint32_t rows = (uint32_t) owned[b].size_y + 4u;
                uint32_t a = 0;
                while (a < rows) {
                    const uint32_t rem = rows - a;
                    const uint32_t h = (a == 0) ? std::min(band_rounds, rem) : (rem <= band_rounds ? rem : band_rounds - 4u);
                    bands.push_back(RowBand{(uint32_t) (b - ps.first), a, a + h, 0u});
                    a += h;
                }
            }
            HIP_TRY(ctx, ws.bands.upload(bands));
            ws.n_bands = (uint32_t) bands.size();
            if (passes.size() == 1) { ws.plan_key = plan_key; ws.plan_n_pix = n_pix; }
        }
        const uint64_t n_rec = n_pix * spp_owned;
        HIP_TRY(ctx, d_rec_a.reserve(n_rec * 16)); HIP_TRY(ctx, d_rec_b.reserve(n_rec * 4));
        AovParams ap;
        std::memset(&ap, 0, sizeof ap);
        float4 *aov_rgb = nullptr;
        if (aov) {
            ap.n_groups = aov->n_groups;
            for (uint32_t g = 0; g < aov->n_groups; ++g) {
                HIP_TRY(ctx, ws.aov_rec[g].reserve(n_rec * 16));
                ap.rec[g] = ws.aov_rec[g].as<float4>(); ap.code[g] = aov->code[g];
            }
            if (aov->rgba) { HIP_TRY(ctx, ws.aov_rec[MSK_MAX_AOV_GROUPS].reserve(n_rec * 16)); aov_rgb = ws.aov_rec[MSK_MAX_AOV_GROUPS].as<float4>(); }
        }
        if (direct) rc = run_direct(sc, stream, prm, direct, spp_owned, d_pix.as<uint4>(), ws.pix_inv.as<uint32_t>(), n_pix, d_rec_a.as<float4>(),
                                    d_rec_b.as<float>(), stats, packed);
        else
        rc = run_wavefront(sc, stream, prm, knobs, spp_owned, d_pix.as<uint4>(), ws.pix_inv.as<uint32_t>(), n_pix, d_rec_a.as<float4>(),
                           d_rec_b.as<float>(), sb, region_size, n_regions, stats, ev, aov ? &ap : nullptr, aov_rgb, packed);
        if (rc) return rc;
        const uint32_t nb = (uint32_t) (ps.second - ps.first);
        // tile of film pixels per thread: 1 wide (adjacent lanes read adjacent records -> full cache lines),
        // TY tall (a record is shared by TY pixels: 5*(TY+4)/TY reads per pixel)
        const int tile_x = (int) env_u32("MSK_RESOLVE_TX", 1), tile_y = (int) env_u32("MSK_RESOLVE_TY", 3);
        const int tiles_x = (bs + 2 * border + tile_x - 1) / tile_x, tiles_y = (bs + 2 * border + tile_y - 1) / tile_y;
        const uint64_t threads = (uint64_t) nb * tiles_x * tiles_y;
        hipEvent_t a = ev.get(), b = ev.get();
        if (a) (void) hipEventRecord(a, stream);
        const dim3 rgrid((uint32_t) ((threads + MSK_BLOCK - 1) / MSK_BLOCK));
#define MSK_RESOLVE(TX, TY) hipLaunchKernelGGL((k_resolve_blocks<TX, TY>), rgrid, dim3(MSK_BLOCK), 0, stream, sc->dev,      \
                           d_blocks.as<BlockInfo>() + ps.first, nb, res_rec, d_rec_b.as<float>(), spp_owned,               \
                           res_buf, buf_stride, tiles_x, tiles_y)
        // the XYZAW records, then every AOV record group through the same ordered replay (same weights, same order)
        for (uint32_t g = 0; g <= n_aov_bufs; ++g) {
            const uint32_t slot = g == 0 ? 0 : (g - 1 < (aov ? aov->n_groups : 0u) ? g - 1 : MSK_MAX_AOV_GROUPS);
            const float4 *res_rec = g == 0 ? d_rec_a.as<float4>() : ws.aov_rec[slot].as<float4>();
            float *res_buf = g == 0 ? d_block_buf.as<float>() : ws.aov_block_buf[slot].as<float>();
            if (packed) {
                if (ws.n_bands)
                    hipLaunchKernelGGL(k_resolve_rows, dim3(ws.n_bands), dim3(MSK_WAVE), (size_t) env_u32("MSK_RESOLVE_PAD_LDS_KB", 0) * 1024, stream, sc->dev, d_blocks.as<BlockInfo>() + ps.first,
                                       ws.bands.as<RowBand>(), ws.n_bands, res_rec, (const uint32_t *) d_rec_b.as<float>(), spp_owned, res_buf, buf_stride);
            }
            else if (tile_x == 2 && tile_y == 2) MSK_RESOLVE(2, 2);
            else if (tile_x == 2 && tile_y == 3) MSK_RESOLVE(2, 3);
            else if (tile_x == 2 && tile_y == 4) MSK_RESOLVE(2, 4);
            else if (tile_x == 1 && tile_y == 1) MSK_RESOLVE(1, 1);
            else if (tile_x == 1 && tile_y == 2) MSK_RESOLVE(1, 2);
            else if (tile_x == 1 && tile_y == 3) MSK_RESOLVE(1, 3);
            else if (tile_x == 1 && tile_y == 6) MSK_RESOLVE(1, 6);
            else MSK_RESOLVE(1, 4);
        }
#undef MSK_RESOLVE
        if (b) (void) hipEventRecord(b, stream);
        ev_resolve.push_back({a, b});
        if ((rc = ctx_sync(ctx, stream, "the film replay of a pass"))) return rc;   // d_pix / records are reused by the next pass
        if (stats) stats->passes++;
    }
    {
        hipEvent_t a = ev.get(), b = ev.get();
        if (a) (void) hipEventRecord(a, stream);
        for (uint32_t g = 0; g <= n_aov_bufs; ++g) {
            const uint32_t slot = g == 0 ? 0 : (g - 1 < (aov ? aov->n_groups : 0u) ? g - 1 : MSK_MAX_AOV_GROUPS);
            FilmOut fo;
            fo.film = d_film; fo.stride = 5 + (int32_t) (aov ? aov->n_channels : 0u);
            for (int c = 0; c < 5; ++c) fo.ch[c] = g == 0 ? c : aov->out_ch[g - 1 < aov->n_groups ? g - 1 : MSK_MAX_AOV_GROUPS][c];
            hipLaunchKernelGGL(k_film_put, dim3((uint32_t) (((size_t) sc->dev.crop_w * sc->dev.crop_h + MSK_BLOCK - 1) / MSK_BLOCK)), dim3(MSK_BLOCK), 0, stream,
                               sc->dev, d_blocks.as<BlockInfo>(), d_block_of.as<int32_t>(), d_spiral.as<uint32_t>(), ob.nbx, ob.nby, bs,
                               g == 0 ? d_block_buf.as<float>() : ws.aov_block_buf[slot].as<float>(), buf_stride, fo);
        }
        if (b) (void) hipEventRecord(b, stream);
        ev_resolve.push_back({a, b});
    }
    if (t_end) (void) hipEventRecord(t_end, stream);
    HIP_TRY(ctx, hipGetLastError());
    if ((rc = ctx_sync(ctx, stream, "Film::put"))) return rc;
    if (stats) {
        if (t_begin && t_end) (void) hipEventElapsedTime(&stats->ms_total, t_begin, t_end);
        sum_events(ev_resolve, &stats->ms_resolve);      // trace / shade were summed group by group in run_wavefront
    }
    return MSK_OK;
}

// The film's copy-back (msk_gpu_render, and a group's summed film).  A caller's array that is PINNED host memory (hipHostMalloc /
// hipHostRegister, a torch pinned tensor) takes the DMA directly: 5 MB in ~0.2 ms.  A pageable one goes through a pinned staging
// buffer kept with the scene (*stage): device -> pinned at link speed, then one host memcpy into the caller's array (~0.4 ms for
// the 5 MB bench film; a pageable hipMemcpy took 2-3 ms).  MSK_COPYBACK_STAGED=1 (tests): always through the staging buffer.
static int film_to_host(msk_ctx *ctx, hipStream_t stream, const void *d_film, float *h_film, size_t bytes, void **stage, size_t *stage_bytes) {
    hipPointerAttribute_t attr;
    const hipError_t ea = hipPointerGetAttributes(&attr, h_film);
    if (ea != hipSuccess) (void) hipGetLastError();                      // (an ordinary malloc'ed pointer is "invalid value" to older runtimes)
    if (ea == hipSuccess && attr.type == hipMemoryTypeHost && !env_u32("MSK_COPYBACK_STAGED", 0)) {
        HIP_TRY(ctx, hipMemcpyAsync(h_film, d_film, bytes, hipMemcpyDeviceToHost, stream));
        return ctx_sync(ctx, stream, "the film's copy-back");
    }
    if (*stage_bytes < bytes) {
        if (*stage) (void) hipHostFree(*stage);
        *stage = nullptr; *stage_bytes = 0;
        if (hipHostMalloc(stage, bytes, hipHostMallocDefault) == hipSuccess) *stage_bytes = bytes;
        else { (void) hipGetLastError(); *stage = nullptr; }
    }
    if (*stage) {
        HIP_TRY(ctx, hipMemcpyAsync(*stage, d_film, bytes, hipMemcpyDeviceToHost, stream));
        if (const int rc = ctx_sync(ctx, stream, "the film's copy-back")) return rc;
        std::memcpy(h_film, *stage, bytes);
    } else {
        HIP_TRY(ctx, hipMemcpy(h_film, d_film, bytes, hipMemcpyDeviceToHost));
    }
    return MSK_OK;
}

extern "C" int msk_gpu_render_device(msk_scene *scene, const msk_render_params *params, float *d_film_xyzaw, void *hip_stream,
                                     msk_stats *stats) {
    if (!scene || !d_film_xyzaw) return fail(scene ? scene->ctx : nullptr, MSK_ERR_INVALID_ARG, "msk_gpu_render_device: NULL argument");
    MSK_REFUSE_LOST(scene->ctx);
    if (scene->ctx->group) return group_render_device(scene, params, d_film_xyzaw, (hipStream_t) hip_stream, stats);
    return render_impl(scene, params, d_film_xyzaw, (hipStream_t) hip_stream, stats);
}

extern "C" int msk_gpu_render(msk_scene *scene, const msk_render_params *params, float *film_xyzaw, msk_stats *stats) {
    if (!scene || !film_xyzaw) return fail(scene ? scene->ctx : nullptr, MSK_ERR_INVALID_ARG, "msk_gpu_render: NULL argument");
    MSK_REFUSE_LOST(scene->ctx);
    if (scene->ctx->group) return group_render(scene, params, film_xyzaw, stats);
    msk_ctx *ctx = scene->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (!scene->ws) scene->ws = new Workspace();
    DevBuf &film = scene->ws->film;
    const size_t bytes = (size_t) scene->dev.crop_w * scene->dev.crop_h * 5 * 4;
    HIP_TRY(ctx, film.reserve(bytes));
    int rc = render_impl(scene, params, film.as<float>(), nullptr, stats);
    if (rc) return rc;
    return film_to_host(ctx, ctx->stream, film.p, film_xyzaw, bytes, &scene->ws->host_film, &scene->ws->host_film_bytes);
}

static const int kAovWidth[6] = {1, 3, 2, 3, 3, 4};
extern "C" uint32_t msk_gpu_aov_channels(const int32_t *aov_types, uint32_t n_aovs) {
    uint32_t n = 0;
    for (uint32_t i = 0; i < n_aovs; ++i) {
        if (!aov_types || aov_types[i] < 0 || aov_types[i] > MSK_AOV_PATH_RGBA) return 0;
        n += (uint32_t) kAovWidth[aov_types[i]];
    }
    return n;
}

extern "C" int msk_gpu_render_aov(msk_scene *scene, const msk_render_params *params, const int32_t *aov_types, uint32_t n_aovs,
                                  float *film, msk_stats *stats) {
    if (!scene || !film || !params || (n_aovs && !aov_types))
        return fail(scene ? scene->ctx : nullptr, MSK_ERR_INVALID_ARG, "msk_gpu_render_aov: NULL argument");
    MSK_REFUSE_LOST(scene->ctx);
    if (scene->ctx->group) return group_render_aov(scene, params, aov_types, n_aovs, film, stats);
    msk_ctx *ctx = scene->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    AovPlan plan;
    for (auto &row : plan.out_ch) for (int &c : row) c = -1;
    // selectors of the primary-hit channels, in film order (AovParams::code)
    static const int first_code[5] = {1, 2, 5, 7, 10};
    std::vector<std::pair<int, int>> prim;        // (selector, film channel)
    int ch = 5;
    for (uint32_t i = 0; i < n_aovs; ++i) {
        const int t = aov_types[i];
        if (t < 0 || t > MSK_AOV_PATH_RGBA) return fail(ctx, MSK_ERR_INVALID_ARG, "Invalid AOV type %d!", t);
        if (t == MSK_AOV_PATH_RGBA) {
            if (plan.rgba) return fail(ctx, MSK_ERR_UNSUPPORTED, "at most one nested integrator is supported by the \"aov\" integrator of this back end");
            plan.rgba = true;
            for (int c = 0; c < 4; ++c) plan.out_ch[MSK_MAX_AOV_GROUPS][c] = ch + c;     // block channel 3 = the weight sum = A
        } else {
            for (int c = 0; c < kAovWidth[t]; ++c) prim.push_back({first_code[t] + c, ch + c});
        }
        ch += kAovWidth[t];
    }
    plan.n_channels = (uint32_t) ch - 5;
    if (prim.size() > 3 * MSK_MAX_AOV_GROUPS)
        return fail(ctx, MSK_ERR_UNSUPPORTED, "too many AOV channels (%zu, at most %d besides the nested integrator)", prim.size(), 3 * MSK_MAX_AOV_GROUPS);
    plan.n_groups = (uint32_t) ((prim.size() + 2) / 3);
    for (size_t k = 0; k < prim.size(); ++k) {
        plan.code[k / 3] |= (uint32_t) prim[k].first << (8 * (k % 3));
        plan.out_ch[k / 3][k % 3] = prim[k].second;
    }
    msk_render_params p = *params;
    if (!plan.rgba) p.max_depth = 0;      // no nested integrator: only the camera ray is traced and XYZ stays 0 (aov.cpp:91)
    if (!scene->ws) scene->ws = new Workspace();
    DevBuf &d_film = scene->ws->film;
    const size_t bytes = (size_t) scene->dev.crop_w * scene->dev.crop_h * (5 + plan.n_channels) * 4;
    HIP_TRY(ctx, d_film.reserve(bytes));
    HIP_TRY(ctx, hipMemsetAsync(d_film.p, 0, bytes, ctx->stream));
    int rc = render_impl(scene, &p, d_film.as<float>(), nullptr, stats, &plan);
    if (rc) return rc;
    HIP_TRY(ctx, hipMemcpy(film, d_film.p, bytes, hipMemcpyDeviceToHost));
    return MSK_OK;
}

// msk_gpu_sample_pixels, and with `direct` msk_gpu_sample_pixels_direct (which honours the sample selectors: msk_gpu.h)
static int sample_pixels_impl(msk_scene *scene, const msk_render_params *prm, uint64_t n_pixels, const int32_t *pixels,
                              float *out_xyz, float *out_pos, const msk_direct_params *direct) {
    msk_ctx *ctx = scene->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc = check_params(ctx, prm, 1);
    if (rc) return rc;
    // every sample 0 .. spp-1 of a listed pixel is rendered (the selectors are ignored below): all of them count against the
    // path state's 20 bits of sample index
    if (!direct && prm->spp > (1u << MSK_DEPTH_SHIFT))
        return fail(ctx, MSK_ERR_UNSUPPORTED, "msk_gpu_sample_pixels: spp %u, at most %u (every sample of a pixel is rendered)",
                    prm->spp, 1u << MSK_DEPTH_SHIFT);
    if (prm->rng_mode != MSK_RNG_COUNTER)
        return fail(ctx, MSK_ERR_UNSUPPORTED, "msk_gpu_sample_pixels: rng_mode %d (a pixel's samples are only addressable with the counter RNG: "
                    "a per-block PCG32 stream is sequential by construction)", prm->rng_mode);
    const int W = scene->dev.width, H = scene->dev.height;
    if (n_pixels >> 32) return fail(ctx, MSK_ERR_INVALID_ARG, "too many pixels");
    // The path state names a sample by its FILM pixel (PathState::id), so a pixel listed twice is rendered once and its
    // samples are copied to every place it is listed at.
    std::vector<uint4> pix;
    std::vector<uint32_t> inv((size_t) W * H, 0xffffffffu), place(n_pixels);
    for (uint64_t i = 0; i < n_pixels; ++i) {
        const int x = pixels[2 * i], y = pixels[2 * i + 1];
        if (x < 0 || y < 0 || x >= W || y >= H) return fail(ctx, MSK_ERR_INVALID_ARG, "pixel (%d,%d) outside the %dx%d film", x, y, W, H);
        const uint32_t f = (uint32_t) (y * W + x);
        if (inv[f] == 0xffffffffu) {
            inv[f] = (uint32_t) pix.size();
            // a "block" of one pixel at (x, y): the kernels take the film coordinates from the block offset (pixel_x / pixel_y)
            pix.push_back(make_uint4(f, 0u, (uint32_t) (x - scene->dev.filter_border), (uint32_t) (y - scene->dev.filter_border)));
        }
        place[i] = inv[f];
    }
    if (n_pixels == 0) return MSK_OK;
    const uint64_t n_listed = n_pixels;
    n_pixels = pix.size();
    msk_render_params p = *prm;
    if (!direct) { p.sample_first = 0; p.sample_stride = 1; }
    const uint32_t spp_out = direct ? (uint32_t) owned_spp(&p) : p.spp;       // samples per listed pixel in the output
    if (spp_out == 0) return MSK_OK;
    const uint64_t n_rec = n_pixels * spp_out;
    const mskplan::RenderKnobs knobs = mskplan::read_render_knobs();
    uint32_t region_size = 0, n_regions = 0;
    StateBufs sb; DevBuf d_pix, d_inv, ra, rb, ox, op;
    if (!direct) {
        mskplan::pool_shape(scene->facts.trace_mode, n_rec, knobs, &region_size, &n_regions);
        HIP_TRY(ctx, sb.alloc((size_t) region_size * n_regions, n_regions));
    }
    HIP_TRY(ctx, d_pix.upload(pix)); HIP_TRY(ctx, d_inv.upload(inv)); HIP_TRY(ctx, ra.alloc(n_rec * 16)); HIP_TRY(ctx, rb.alloc(n_rec * 4));
    HIP_TRY(ctx, ox.alloc(n_rec * 12)); HIP_TRY(ctx, op.alloc(n_rec * 8));
    EventPool ev{ctx, 0};
    // a lost context (the watchdog gave up): the local buffers are dropped without hipFree, which would wait for the device
    auto sb_leak = [&]() { if (ctx->lost) { sb.leak(); for (DevBuf *b : {&d_pix, &d_inv, &ra, &rb, &ox, &op}) b->leak(); } };
    if (direct) rc = run_direct(scene, ctx->stream, &p, direct, spp_out, d_pix.as<uint4>(), d_inv.as<uint32_t>(), n_pixels, ra.as<float4>(), rb.as<float>(), nullptr, false);
    else
    rc = run_wavefront(scene, ctx->stream, &p, knobs, p.spp, d_pix.as<uint4>(), d_inv.as<uint32_t>(), n_pixels, ra.as<float4>(), rb.as<float>(), sb,
                       region_size, n_regions, nullptr, ev);
    if (rc) { sb_leak(); return rc; }
    hipLaunchKernelGGL(k_export_records, dim3((uint32_t) ((n_rec + 255) / 256)), dim3(256), 0, ctx->stream, ra.as<float4>(),
                       rb.as<float>(), n_pixels, spp_out, ox.as<float>(), op.as<float>());
    if ((rc = ctx_sync(ctx, ctx->stream, "k_export_records"))) { sb_leak(); return rc; }
    std::vector<float> hx((size_t) n_rec * 3), hp(out_pos ? (size_t) n_rec * 2 : 0);
    HIP_TRY(ctx, hipMemcpy(hx.data(), ox.p, n_rec * 12, hipMemcpyDeviceToHost));
    if (out_pos) HIP_TRY(ctx, hipMemcpy(hp.data(), op.p, n_rec * 8, hipMemcpyDeviceToHost));
    for (uint64_t i = 0; i < n_listed; ++i) {
        std::memcpy(out_xyz + i * spp_out * 3, hx.data() + (size_t) place[i] * spp_out * 3, (size_t) spp_out * 12);
        if (out_pos) std::memcpy(out_pos + i * spp_out * 2, hp.data() + (size_t) place[i] * spp_out * 2, (size_t) spp_out * 8);
    }
    return MSK_OK;
}

extern "C" int msk_gpu_sample_pixels(msk_scene *scene, const msk_render_params *prm, uint64_t n_pixels, const int32_t *pixels,
                                     float *out_xyz, float *out_pos) {
    if (!scene || !pixels || !out_xyz) return fail(scene ? scene->ctx : nullptr, MSK_ERR_INVALID_ARG, "msk_gpu_sample_pixels: NULL argument");
    MSK_REFUSE_LOST(scene->ctx);
    if (scene->ctx->group) {             // sub-stage entry points of a group run on its first member
        const int rc = msk_gpu_sample_pixels(scene->parts[0], prm, n_pixels, pixels, out_xyz, out_pos);
        return rc ? group_fail(scene->ctx, 0, rc) : MSK_OK;
    }
    return sample_pixels_impl(scene, prm, n_pixels, pixels, out_xyz, out_pos, nullptr);
}

// ---- the "direct" integrator (msk_gpu.h: msk_direct_params; msk_direct.h) ----------------------------------------------------------
// What the three calls refuse before anything runs, and the parameters they render with: rr_depth and max_depth are ignored.
static int check_direct(msk_scene *scene, const msk_render_params *prm, const msk_direct_params *d, const char *who, msk_render_params *out) {
    msk_ctx *ctx = scene->ctx;
    if (!prm || !d) return fail(ctx, MSK_ERR_INVALID_ARG, "%s: NULL argument", who);
    if (ctx->group)
        return fail(ctx, MSK_ERR_UNSUPPORTED, "%s: group contexts (msk_gpu_init with n > 1) are not supported by the \"direct\" integrator; "
                    "run one process per GPU and shard the samples with sample_first / sample_stride", who);
    if (scene->facts.has_mask)
        return fail(ctx, MSK_ERR_UNSUPPORTED, "%s: the scene holds a `mask` BSDF, which the \"direct\" integrator does not support "
                    "(a cutout would be a black hole in a one-bounce integrator; use \"path\")", who);
    if (scene->facts.has_plastic) {
        for (int32_t type : scene->bsdf_types)
            if (type == MSK_BSDF_ROUGHPLASTIC)
                return fail(ctx, MSK_ERR_UNSUPPORTED, "%s: the scene holds a `roughplastic` BSDF, which the \"direct\" integrator does not support "
                            "(its kernel carries neither the GGX coat nor the diffuse base under it; use \"path\")", who);
        return fail(ctx, MSK_ERR_UNSUPPORTED, "%s: the scene holds a `plastic` BSDF, which the \"direct\" integrator does not support "
                    "(its kernel carries neither the coat's delta lobe nor the diffuse base under it; use \"path\")", who);
    }
    if (prm->rng_mode == MSK_RNG_PCG_BLOCK)
        return fail(ctx, MSK_ERR_UNSUPPORTED, "%s: MSK_RNG_PCG_BLOCK is not supported by the \"direct\" integrator (it uses MSK_RNG_COUNTER)", who);
    if (d->light_samples > mskplan::kDirectMaxSamples)
        return fail(ctx, MSK_ERR_INVALID_ARG, "%s: \"light_samples\" is %u, at most %u", who, d->light_samples, mskplan::kDirectMaxSamples);
    if (d->bsdf_samples > mskplan::kDirectMaxSamples)
        return fail(ctx, MSK_ERR_INVALID_ARG, "%s: \"bsdf_samples\" is %u, at most %u", who, d->bsdf_samples, mskplan::kDirectMaxSamples);
    if (d->light_samples == 0 && d->bsdf_samples == 0)
        return fail(ctx, MSK_ERR_INVALID_ARG, "%s: \"light_samples\" and \"bsdf_samples\" must not both be 0", who);
    *out = *prm;
    out->rr_depth = 5; out->max_depth = -1;
    return MSK_OK;
}

extern "C" int msk_gpu_render_direct_device(msk_scene *scene, const msk_render_params *params, const msk_direct_params *direct,
                                            float *d_film_xyzaw, void *hip_stream, msk_stats *stats) {
    if (!scene || !d_film_xyzaw) return fail(scene ? scene->ctx : nullptr, MSK_ERR_INVALID_ARG, "msk_gpu_render_direct_device: NULL argument");
    MSK_REFUSE_LOST(scene->ctx);
    msk_render_params p;
    if (int rc = check_direct(scene, params, direct, "msk_gpu_render_direct_device", &p)) return rc;
    return render_impl(scene, &p, d_film_xyzaw, (hipStream_t) hip_stream, stats, nullptr, direct);
}

extern "C" int msk_gpu_render_direct(msk_scene *scene, const msk_render_params *params, const msk_direct_params *direct,
                                     float *film_xyzaw, msk_stats *stats) {
    if (!scene || !film_xyzaw) return fail(scene ? scene->ctx : nullptr, MSK_ERR_INVALID_ARG, "msk_gpu_render_direct: NULL argument");
    MSK_REFUSE_LOST(scene->ctx);
    msk_render_params p;
    if (int rc = check_direct(scene, params, direct, "msk_gpu_render_direct", &p)) return rc;
    msk_ctx *ctx = scene->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (!scene->ws) scene->ws = new Workspace();
    DevBuf &film = scene->ws->film;
    const size_t bytes = (size_t) scene->dev.crop_w * scene->dev.crop_h * 5 * 4;
    HIP_TRY(ctx, film.reserve(bytes));
    if (int rc = render_impl(scene, &p, film.as<float>(), nullptr, stats, nullptr, direct)) return rc;
    return film_to_host(ctx, ctx->stream, film.p, film_xyzaw, bytes, &scene->ws->host_film, &scene->ws->host_film_bytes);
}

extern "C" int msk_gpu_sample_pixels_direct(msk_scene *scene, const msk_render_params *params, const msk_direct_params *direct,
                                            uint64_t n_pixels, const int32_t *pixels, float *out_xyz, float *out_pos) {
    if (!scene || !pixels || !out_xyz) return fail(scene ? scene->ctx : nullptr, MSK_ERR_INVALID_ARG, "msk_gpu_sample_pixels_direct: NULL argument");
    MSK_REFUSE_LOST(scene->ctx);
    msk_render_params p;
    if (int rc = check_direct(scene, params, direct, "msk_gpu_sample_pixels_direct", &p)) return rc;
    return sample_pixels_impl(scene, &p, n_pixels, pixels, out_xyz, out_pos, direct);
}

// ------------------------------------------------------------------------------------------
// the probe calls: n points through one small kernel that calls what the render kernels call (msk_gpu.h).  Each entry point keeps its
// own argument checks and refusals; the two helpers are what they all do besides.
// ------------------------------------------------------------------------------------------
struct ProbeIn { const void *host; size_t bytes; };      // host == nullptr: the call does not use this one; the kernel gets a null pointer
struct ProbeOut { void *host; size_t bytes; };

// One probe kernel over n points on the scene's device: the inputs go up, `launch(in, out, grid)` starts the kernel on ctx->stream with
// the device pointers (in the order of the two lists) and returns what allocations of its own returned, the wait is timed under the
// kernel's name, the outputs come down.  n == 0 succeeds with nothing done.  After a wait that fails nothing is freed (DevBuf::leak).
template <class Launch>
static int run_probe(msk_scene *scene, const char *kernel, uint64_t n, std::initializer_list<ProbeIn> ins, std::initializer_list<ProbeOut> outs, Launch &&launch) {
    msk_ctx *ctx = scene->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (n == 0) return MSK_OK;
    std::vector<DevBuf> bufs(ins.size() + outs.size());
    std::vector<void *> d;
    for (const ProbeIn &b : ins) {
        DevBuf &buf = bufs[d.size()];
        if (b.host) { HIP_TRY(ctx, buf.alloc(b.bytes)); HIP_TRY(ctx, hipMemcpy(buf.p, b.host, b.bytes, hipMemcpyHostToDevice)); }
        d.push_back(buf.p);
    }
    for (const ProbeOut &b : outs) {
        DevBuf &buf = bufs[d.size()];
        if (b.host) HIP_TRY(ctx, buf.alloc(b.bytes));
        d.push_back(buf.p);
    }
    void *const *d_out = d.data() + ins.size();
    const uint32_t grid = (uint32_t) std::min<uint64_t>((n + MSK_BLOCK - 1) / MSK_BLOCK, 4096);
    HIP_TRY(ctx, launch(d.data(), d_out, grid));
    HIP_TRY(ctx, hipGetLastError());
    if (int rcw = ctx_sync(ctx, ctx->stream, kernel)) { for (DevBuf &b : bufs) b.leak(); return rcw; }
    size_t k = 0;
    for (const ProbeOut &b : outs) {
        if (b.host) HIP_TRY(ctx, hipMemcpy(b.host, d_out[k], b.bytes, hipMemcpyDeviceToHost));
        ++k;
    }
    return MSK_OK;
}
// a probe of a group's scene runs on its first member's; a failure there is reported as the group's
template <class F>
static int on_first_part(msk_scene *scene, F &&f) {
    if (!scene->ctx->group) return f(scene);
    const int rc = f(scene->parts[0]);
    return rc ? group_fail(scene->ctx, 0, rc) : MSK_OK;
}

static int trace_batch(msk_scene *scene, uint64_t n, const float *rays, float *out_hit, uint8_t *out_any) {
    msk_ctx *ctx = scene->ctx;
    MSK_REFUSE_LOST(ctx);
    DevBuf d_ovf;                 // the lanes' overflow stacks: sized by the grid
    const int rc = run_probe(scene, "k_trace_batch", n, {{rays, n * 32}}, {{out_any ? (void *) out_any : (void *) out_hit, out_any ? n : n * 16}},
                             [&](void *const *in, void *const *out, uint32_t grid) {
        if (scene->dev.stack_total > scene->dev.stack_entries)
            if (hipError_t e = d_ovf.alloc((size_t) (scene->dev.stack_total - scene->dev.stack_entries) * grid * MSK_BLOCK * 4)) return e;
        with_trace_mode(scene->facts.trace_mode, [&](auto m) {
            hipLaunchKernelGGL(k_trace_batch<decltype(m)::value>, dim3(grid), dim3(MSK_BLOCK), scene->facts.trace_lds_bytes, ctx->stream, scene->dev,
                               (const float4 *) in[0], n, out_any ? nullptr : (float4 *) out[0], out_any ? (uint8_t *) out[0] : nullptr, d_ovf.as<uint32_t>());
        });
        return hipSuccess;
    });
    if (ctx->lost) d_ovf.leak();
    return rc;
}
extern "C" int msk_gpu_trace_closest(msk_scene *scene, uint64_t n, const float *rays, float *out_hit) {
    if (!scene || (n && (!rays || !out_hit))) return fail(scene ? scene->ctx : nullptr, MSK_ERR_INVALID_ARG, "msk_gpu_trace_closest: NULL argument");
    return on_first_part(scene, [&](msk_scene *s) { return trace_batch(s, n, rays, out_hit, nullptr); });
}
extern "C" int msk_gpu_trace_any(msk_scene *scene, uint64_t n, const float *rays, uint8_t *out_occluded) {
    if (!scene || (n && (!rays || !out_occluded))) return fail(scene ? scene->ctx : nullptr, MSK_ERR_INVALID_ARG, "msk_gpu_trace_any: NULL argument");
    return on_first_part(scene, [&](msk_scene *s) { return trace_batch(s, n, rays, nullptr, out_occluded); });
}

static int eval_texture(msk_scene *scene, uint32_t texture, uint64_t n, const float *uv, const float *wavelengths, float *out) {
    msk_ctx *ctx = scene->ctx;
    MSK_REFUSE_LOST(ctx);
    if (texture < 1 || texture > scene->n_textures)
        return fail(ctx, MSK_ERR_INVALID_ARG, "msk_gpu_eval_texture: texture %u out of range (1 .. %u)", texture, scene->n_textures);
    return run_probe(scene, "k_eval_texture", n, {{uv, n * 8}, {wavelengths, n * 16}}, {{out, n * 16}}, [&](void *const *in, void *const *o, uint32_t grid) {
        hipLaunchKernelGGL(k_eval_texture, dim3(grid), dim3(MSK_BLOCK), 0, ctx->stream, scene->dev, scene->tex_base + (texture - 1) * 3, n,
                           (const float2 *) in[0], (const float4 *) in[1], (float4 *) o[0]);
        return hipSuccess;
    });
}
extern "C" int msk_gpu_eval_texture(msk_scene *scene, uint32_t texture, uint64_t n, const float *uv, const float *wavelengths, float *out) {
    if (!scene || (n && (!uv || !wavelengths || !out))) return fail(scene ? scene->ctx : nullptr, MSK_ERR_INVALID_ARG, "msk_gpu_eval_texture: NULL argument");
    return on_first_part(scene, [&](msk_scene *s) { return eval_texture(s, texture, n, uv, wavelengths, out); });
}

// msk_gpu_env_eval (sample == 0: `in` = n * 3 directions) / msk_gpu_env_sample (sample == 1: `in` = n * 2 random numbers)
static int env_probe(msk_scene *scene, const char *who, uint32_t sample, uint64_t n, const float *in, const float *wavelengths, float *out_rad, float *out_dir,
                     float *out_uv, float *out_pdf) {
    msk_ctx *ctx = scene->ctx;
    MSK_REFUSE_LOST(ctx);
    if (!scene->facts.has_envmap) return fail(ctx, MSK_ERR_INVALID_ARG, "%s: the scene has no envmap emitter", who);
    return run_probe(scene, "k_env_probe", n, {{in, n * (sample ? 2 : 3) * 4}, {wavelengths, n * 16}},
                     {{out_rad, n * 16}, {out_dir, n * 12}, {out_uv, n * 8}, {out_pdf, n * 4}}, [&](void *const *i, void *const *o, uint32_t grid) {
        hipLaunchKernelGGL(k_env_probe, dim3(grid), dim3(MSK_BLOCK), 0, ctx->stream, scene->dev, sample, n, (const float *) i[0], (const float4 *) i[1],
                           (float4 *) o[0], (float *) o[1], (float2 *) o[2], (float *) o[3]);
        return hipSuccess;
    });
}
extern "C" int msk_gpu_env_eval(msk_scene *scene, uint64_t n, const float *dirs, const float *wavelengths, float *out_radiance, float *out_pdf) {
    if (!scene || (n && (!dirs || !wavelengths || !out_radiance || !out_pdf))) return fail(scene ? scene->ctx : nullptr, MSK_ERR_INVALID_ARG, "msk_gpu_env_eval: NULL argument");
    return on_first_part(scene, [&](msk_scene *s) { return env_probe(s, "msk_gpu_env_eval", 0, n, dirs, wavelengths, out_radiance, nullptr, nullptr, out_pdf); });
}
extern "C" int msk_gpu_env_sample(msk_scene *scene, uint64_t n, const float *u, float *out_dir, float *out_uv, float *out_pdf) {
    if (!scene || (n && (!u || !out_dir || !out_uv || !out_pdf))) return fail(scene ? scene->ctx : nullptr, MSK_ERR_INVALID_ARG, "msk_gpu_env_sample: NULL argument");
    return on_first_part(scene, [&](msk_scene *s) { return env_probe(s, "msk_gpu_env_sample", 1, n, u, nullptr, nullptr, out_dir, out_uv, out_pdf); });
}

// msk_gpu_point_sample (conductor == 0: `in` = n * 3 reference points, two outputs) / msk_gpu_conductor_sample (1: `in` = n cosines,
// out_a unused) / msk_gpu_light_sample (2: as 0, for a spot or directional emitter)
static int delta_probe(msk_scene *scene, const char *who, uint32_t conductor, uint32_t index, uint64_t n, const float *in, const float *wavelengths, float *out_a, float *out_b) {
    msk_ctx *ctx = scene->ctx;
    MSK_REFUSE_LOST(ctx);
    if (conductor == 2u) {
        if (index >= scene->emitter_types.size() || (scene->emitter_types[index] != MSK_EMITTER_SPOT && scene->emitter_types[index] != MSK_EMITTER_DIRECTIONAL))
            return fail(ctx, MSK_ERR_INVALID_ARG, "%s: emitter %u is neither a spot nor a directional emitter of this scene", who, index);
    } else
    if (!scene->facts.has_delta) return fail(ctx, MSK_ERR_INVALID_ARG, "%s: the scene holds neither a point emitter nor a conductor", who);
    else if (conductor) {
        if (index >= scene->bsdf_types.size() || scene->bsdf_types[index] != MSK_BSDF_CONDUCTOR) return fail(ctx, MSK_ERR_INVALID_ARG, "%s: bsdf %u is not a conductor of this scene", who, index);
    } else if (index >= scene->emitter_types.size() || scene->emitter_types[index] != MSK_EMITTER_POINT) return fail(ctx, MSK_ERR_INVALID_ARG, "%s: emitter %u is not a point emitter of this scene", who, index);
    return run_probe(scene, "k_delta_probe", n, {{in, n * (conductor == 1u ? 1 : 3) * 4}, {wavelengths, n * 16}}, {{out_a, n * 16}, {out_b, n * 16}},
                     [&](void *const *i, void *const *o, uint32_t grid) {
        hipLaunchKernelGGL(k_delta_probe, dim3(grid), dim3(MSK_BLOCK), 0, ctx->stream, scene->dev, conductor, index, n, (const float *) i[0], (const float4 *) i[1],
                           (float4 *) o[0], (float4 *) o[1]);
        return hipSuccess;
    });
}
extern "C" int msk_gpu_point_sample(msk_scene *scene, uint32_t emitter, uint64_t n, const float *ref_points, const float *wavelengths, float *out_d_dist, float *out_value) {
    if (!scene || (n && (!ref_points || !wavelengths || !out_d_dist || !out_value))) return fail(scene ? scene->ctx : nullptr, MSK_ERR_INVALID_ARG, "msk_gpu_point_sample: NULL argument");
    return on_first_part(scene, [&](msk_scene *s) { return delta_probe(s, "msk_gpu_point_sample", 0, emitter, n, ref_points, wavelengths, out_d_dist, out_value); });
}
extern "C" int msk_gpu_light_sample(msk_scene *scene, uint32_t emitter, uint64_t n, const float *ref_points, const float *wavelengths, float *out_d_dist, float *out_value) {
    if (!scene || (n && (!ref_points || !wavelengths || !out_d_dist || !out_value))) return fail(scene ? scene->ctx : nullptr, MSK_ERR_INVALID_ARG, "msk_gpu_light_sample: NULL argument");
    return on_first_part(scene, [&](msk_scene *s) { return delta_probe(s, "msk_gpu_light_sample", 2, emitter, n, ref_points, wavelengths, out_d_dist, out_value); });
}
extern "C" int msk_gpu_conductor_sample(msk_scene *scene, uint32_t bsdf, uint64_t n, const float *cos_theta_i, const float *wavelengths, float *out_value) {
    if (!scene || (n && (!cos_theta_i || !wavelengths || !out_value))) return fail(scene ? scene->ctx : nullptr, MSK_ERR_INVALID_ARG, "msk_gpu_conductor_sample: NULL argument");
    return on_first_part(scene, [&](msk_scene *s) { return delta_probe(s, "msk_gpu_conductor_sample", 1, bsdf, n, cos_theta_i, wavelengths, nullptr, out_value); });
}

// msk_gpu_camera_sample: k_camera_probe, with or without the lens
static int camera_probe(msk_scene *scene, uint64_t n, const float *film_pos, const float *aperture_u, float *out_rays) {
    msk_ctx *ctx = scene->ctx;
    MSK_REFUSE_LOST(ctx);
    const bool lens = scene->facts.has_lens;
    if (n && lens && !aperture_u) return fail(ctx, MSK_ERR_INVALID_ARG, "msk_gpu_camera_sample: a scene with a `thinlens` sensor needs aperture_u");
    return run_probe(scene, "k_camera_probe", n, {{film_pos, n * 8}, {lens ? aperture_u : nullptr, n * 8}}, {{out_rays, n * 32}},
                     [&](void *const *in, void *const *o, uint32_t grid) {
        if (lens) hipLaunchKernelGGL(k_camera_probe<true>, dim3(grid), dim3(MSK_BLOCK), 0, ctx->stream, scene->dev, n, (const float2 *) in[0], (const float2 *) in[1], (float4 *) o[0]);
        else hipLaunchKernelGGL(k_camera_probe<false>, dim3(grid), dim3(MSK_BLOCK), 0, ctx->stream, scene->dev, n, (const float2 *) in[0], (const float2 *) nullptr, (float4 *) o[0]);
        return hipSuccess;
    });
}
extern "C" int msk_gpu_camera_sample(msk_scene *scene, uint64_t n, const float *film_pos, const float *aperture_u, float *out_rays) {
    if (!scene || (n && (!film_pos || !out_rays))) return fail(scene ? scene->ctx : nullptr, MSK_ERR_INVALID_ARG, "msk_gpu_camera_sample: NULL argument");
    return on_first_part(scene, [&](msk_scene *s) { return camera_probe(s, n, film_pos, aperture_u, out_rays); });
}

// msk_gpu_mask_sample (eval == 0: in_b = {sample1, u.x, u.y}, three outputs) / msk_gpu_mask_eval (in_b = wo; out_a = n * 2 {a, pdf}, no out_c);
// msk_gpu_plastic_sample / msk_gpu_plastic_eval and the roughplastic pair (plastic = MSK_BSDF_PLASTIC / MSK_BSDF_ROUGHPLASTIC: the same kernel on an entry that
// must be of that type, in a scene with or without a mask)
static int mask_probe(msk_scene *scene, const char *who, uint32_t eval, uint32_t bsdf, uint64_t n, const float *uv, const float *in_a, const float *in_b,
                      const float *wavelengths, float *out_a, float *out_b, float *out_c, int plastic = 0) {
    msk_ctx *ctx = scene->ctx;
    MSK_REFUSE_LOST(ctx);
    if (!plastic && !scene->facts.has_mask) return fail(ctx, MSK_ERR_INVALID_ARG, "%s: the scene holds no mask", who);
    if (bsdf >= scene->bsdf_types.size()) return fail(ctx, MSK_ERR_INVALID_ARG, "%s: bsdf %u out of range (the scene has %zu)", who, bsdf, scene->bsdf_types.size());
    if (plastic && scene->bsdf_types[bsdf] != plastic)
        return fail(ctx, MSK_ERR_INVALID_ARG, "%s: bsdf %u is not a %s of this scene", who, bsdf, plastic == MSK_BSDF_ROUGHPLASTIC ? "roughplastic" : "plastic");
    std::vector<float> tmp(eval ? n * 4 : 0);           // eval: the kernel's float4 {a, pdf, 0, 0}, of which the caller gets two floats
    const int rc = run_probe(scene, "k_mask_probe", n, {{uv, n * 8}, {in_a, n * 12}, {in_b, n * 12}, {wavelengths, n * 16}},
                             {{eval ? tmp.data() : out_a, n * 16}, {out_b, n * 16}, {out_c, n * 16}}, [&](void *const *in, void *const *o, uint32_t grid) {
        hipLaunchKernelGGL(k_mask_probe, dim3(grid), dim3(MSK_BLOCK), 0, ctx->stream, scene->dev, eval, bsdf, n, (const float *) in[0], (const float *) in[1],
                           (const float *) in[2], (const float4 *) in[3], (float4 *) o[0], (float4 *) o[1], (float4 *) o[2]);
        return hipSuccess;
    });
    if (rc == MSK_OK && eval) for (uint64_t i = 0; i < n; ++i) { out_a[i * 2] = tmp[i * 4]; out_a[i * 2 + 1] = tmp[i * 4 + 1]; }
    return rc;
}
extern "C" int msk_gpu_mask_sample(msk_scene *scene, uint32_t bsdf, uint64_t n, const float *uv, const float *wi, const float *sample1_u, const float *wavelengths,
                                   float *out_wo_pdf, float *out_value, float *out_flags) {
    if (!scene || (n && (!uv || !wi || !sample1_u || !wavelengths || !out_wo_pdf || !out_value || !out_flags)))
        return fail(scene ? scene->ctx : nullptr, MSK_ERR_INVALID_ARG, "msk_gpu_mask_sample: NULL argument");
    return on_first_part(scene, [&](msk_scene *s) { return mask_probe(s, "msk_gpu_mask_sample", 0, bsdf, n, uv, wi, sample1_u, wavelengths, out_wo_pdf, out_value, out_flags); });
}
extern "C" int msk_gpu_mask_eval(msk_scene *scene, uint32_t bsdf, uint64_t n, const float *uv, const float *wi, const float *wo, const float *wavelengths,
                                 float *out_a_pdf, float *out_value) {
    if (!scene || (n && (!uv || !wi || !wo || !wavelengths || !out_a_pdf || !out_value)))
        return fail(scene ? scene->ctx : nullptr, MSK_ERR_INVALID_ARG, "msk_gpu_mask_eval: NULL argument");
    return on_first_part(scene, [&](msk_scene *s) { return mask_probe(s, "msk_gpu_mask_eval", 1, bsdf, n, uv, wi, wo, wavelengths, out_a_pdf, out_value, nullptr); });
}
extern "C" int msk_gpu_plastic_sample(msk_scene *scene, uint32_t bsdf, uint64_t n, const float *uv, const float *wi, const float *sample1_u, const float *wavelengths,
                                      float *out_wo_pdf, float *out_value, float *out_flags) {
    if (!scene || (n && (!uv || !wi || !sample1_u || !wavelengths || !out_wo_pdf || !out_value || !out_flags)))
        return fail(scene ? scene->ctx : nullptr, MSK_ERR_INVALID_ARG, "msk_gpu_plastic_sample: NULL argument");
    return on_first_part(scene, [&](msk_scene *s) { return mask_probe(s, "msk_gpu_plastic_sample", 0, bsdf, n, uv, wi, sample1_u, wavelengths, out_wo_pdf, out_value, out_flags, MSK_BSDF_PLASTIC); });
}
extern "C" int msk_gpu_plastic_eval(msk_scene *scene, uint32_t bsdf, uint64_t n, const float *uv, const float *wi, const float *wo, const float *wavelengths,
                                    float *out_a_pdf, float *out_value) {
    if (!scene || (n && (!uv || !wi || !wo || !wavelengths || !out_a_pdf || !out_value)))
        return fail(scene ? scene->ctx : nullptr, MSK_ERR_INVALID_ARG, "msk_gpu_plastic_eval: NULL argument");
    return on_first_part(scene, [&](msk_scene *s) { return mask_probe(s, "msk_gpu_plastic_eval", 1, bsdf, n, uv, wi, wo, wavelengths, out_a_pdf, out_value, nullptr, MSK_BSDF_PLASTIC); });
}
extern "C" int msk_gpu_roughplastic_sample(msk_scene *scene, uint32_t bsdf, uint64_t n, const float *uv, const float *wi, const float *sample1_u, const float *wavelengths,
                                           float *out_wo_pdf, float *out_value, float *out_flags) {
    if (!scene || (n && (!uv || !wi || !sample1_u || !wavelengths || !out_wo_pdf || !out_value || !out_flags)))
        return fail(scene ? scene->ctx : nullptr, MSK_ERR_INVALID_ARG, "msk_gpu_roughplastic_sample: NULL argument");
    return on_first_part(scene, [&](msk_scene *s) { return mask_probe(s, "msk_gpu_roughplastic_sample", 0, bsdf, n, uv, wi, sample1_u, wavelengths, out_wo_pdf, out_value, out_flags, MSK_BSDF_ROUGHPLASTIC); });
}
extern "C" int msk_gpu_roughplastic_eval(msk_scene *scene, uint32_t bsdf, uint64_t n, const float *uv, const float *wi, const float *wo, const float *wavelengths,
                                         float *out_a_pdf, float *out_value) {
    if (!scene || (n && (!uv || !wi || !wo || !wavelengths || !out_a_pdf || !out_value)))
        return fail(scene ? scene->ctx : nullptr, MSK_ERR_INVALID_ARG, "msk_gpu_roughplastic_eval: NULL argument");
    return on_first_part(scene, [&](msk_scene *s) { return mask_probe(s, "msk_gpu_roughplastic_eval", 1, bsdf, n, uv, wi, wo, wavelengths, out_a_pdf, out_value, nullptr, MSK_BSDF_ROUGHPLASTIC); });
}
// the packed {fdr_int, ssw} of a plastic or roughplastic entry: host memory, no device work
extern "C" int msk_gpu_plastic_constants(msk_scene *scene, uint32_t bsdf, float out[2]) {
    if (!scene || !out) return fail(scene ? scene->ctx : nullptr, MSK_ERR_INVALID_ARG, "msk_gpu_plastic_constants: NULL argument");
    return on_first_part(scene, [&](msk_scene *s) {
        if (bsdf >= s->bsdf_types.size() || (s->bsdf_types[bsdf] != MSK_BSDF_PLASTIC && s->bsdf_types[bsdf] != MSK_BSDF_ROUGHPLASTIC))
            return fail(s->ctx, MSK_ERR_INVALID_ARG, "msk_gpu_plastic_constants: bsdf %u is not a plastic of this scene", bsdf);
        out[0] = s->plastic_constants[(size_t) bsdf * 2]; out[1] = s->plastic_constants[(size_t) bsdf * 2 + 1];
        return (int) MSK_OK;
    });
}
