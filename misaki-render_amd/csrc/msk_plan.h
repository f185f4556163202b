// msk_plan.h — what a render launches, decided once per call and on the host alone: the environment knobs of the wavefront
// driver (RenderKnobs), the shape of the path pool (pool_shape), which instantiation of the shading, traversal and fused kernels
// runs with how much LDS (LaunchPlan), and how a pass's samples and regions are dealt out (region_share, part_ranges).
// And what a scene's creation decides, once per scene: its environment knobs (SceneKnobs), where the shading tables live
// (place_tables) and which form of the tree is walked from where (place_tree); the scene keeps the outcome as its SceneFacts.
// Plain C++17, no HIP: msk_gpu.hip only picks the instantiation the plan names (launch_shade / launch_trace / launch_fused) and
// uploads the tree form the placement names; tests/native/launch_plan_check.cpp and tests/native/scene_tables_check.cpp check
// every decision on a CPU.  (The tables themselves are packed by msk_scene_tables.h; the layout constants are msk_layout.h's.)
#pragma once
#include "msk_layout.h"
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace mskplan {

// The tree the traversal kernels walk: msk_scene::trace_mode and the kernels' MODE parameter hold these values.
enum TraceMode : int {
    TRACE_BIN_LDS    = 0,    // binary tree, staged in LDS with the triangles (a scene of MSK_LDS_SCENE_KB or less)
    TRACE_BIN_HBM    = 1,    // binary tree in HBM/L2 (MSK_WIDE_BVH=0, or a root that is a leaf)
    TRACE_WIDE4      = 2,    // 4-wide tree, 128-byte nodes with full-precision child boxes (MSK_QUANT_BVH=0)
    TRACE_WIDE4_LDS  = 3,    // 4-wide tree staged in LDS (the MSK_WIDE_LDS experiment); never walked with lane replacement
    TRACE_WIDE8      = 4,    // 8-wide tree, quantised child boxes in 128-byte nodes (MSK_WIDE_BVH=8)
    TRACE_WIDE4_BYTE = 5,    // 4-wide tree, 64-byte nodes with byte-quantised boxes (MSK_QUANT_BVH=1; the default of rounds 3-4)
    TRACE_WIDE4_HALF = 6     // 4-wide tree, 80-byte nodes with half-float boxes: the default for a tree in HBM (MSK_QUANT_BVH=2)
};
// the tree stays in HBM/L2: a capped LDS stack with an overflow array, the larger pool, lane replacement by default
constexpr bool tree_in_hbm(int mode) { return mode == TRACE_BIN_HBM || mode == TRACE_WIDE4 || mode == TRACE_WIDE8 || mode == TRACE_WIDE4_BYTE || mode == TRACE_WIDE4_HALF; }

constexpr size_t kWavesPerBlock = MSK_BLOCK / MSK_WAVE;
constexpr size_t kDoneQueueBytes = kWavesPerBlock * MSK_DONE_Q_F4 * 16;     // the waves' done-queues of k_shade_gen: MSK_DONE_Q_F4 float4 per wave
constexpr size_t kLdsLimit = 64 * 1024;
constexpr size_t kLdsTablesLimit = 40 * 1024;                               // every shading table in LDS up to this size (place_tables)
constexpr size_t kSmallTablesLimit = (size_t) MSK_SMALL_TABLES_KB * 1024;   // ... else the small ones, up to this size

inline uint32_t env_u32(const char *name, uint32_t def) {
    const char *v = getenv(name);
    return v && *v ? (uint32_t) strtoul(v, nullptr, 10) : def;
}
// the same where the default depends on the scene: -1 = unset (or empty)
inline long long env_opt(const char *name) {
    const char *v = getenv(name);
    return v && *v ? (long long) (uint32_t) strtoul(v, nullptr, 10) : -1;
}

// Every environment knob of the wavefront driver, read ONCE per render call by the calling thread and never kept between calls
// (the tests set knobs between two renders of one process).  The knobs of scene creation: SceneKnobs, below; those of the film
// replay, of the watchdog (msk_watchdog.h) and of group contexts (msk_multi.h) are read where they are used.
struct RenderKnobs {
    long long regions = -1, region_size = -1;   // MSK_REGIONS, MSK_REGION_SIZE; -1 = unset: the default of the tree's place (pool_shape)
    uint32_t streams = 4, stream_skew = 10;     // MSK_STREAMS, MSK_STREAM_SKEW (per cent)
    uint32_t host_threads = 1;                  // MSK_HOST_THREADS
    uint32_t sync_group = 8;                    // MSK_SYNC_GROUP
    uint32_t timing_every = 1;                  // MSK_TIMING_EVERY (at least 1)
    bool sort = true;                           // MSK_SORT
    bool camera_cull = true;                    // MSK_CAMERA_CULL
    bool force_general_shade = false;           // MSK_FORCE_GENERAL_SHADE
    bool fused = false, fused_hbm = true;       // MSK_FUSED, MSK_FUSED_HBM
    uint32_t fused_iters = 16;                  // MSK_FUSED_ITERS (at least 1)
    long long fused_tail_pct = -1;              // MSK_FUSED_TAIL_PCT; -1 = unset: 2 with k_wavefront_h, else 10
    int trace_refill = -1;                      // MSK_TRACE_REFILL; -1 = unset, which is NOT 0: only an unset knob leaves k_trace_q on
    int trace_quantum = 3;                      // MSK_TRACE_QUANTUM   (4 until round 5's better tree: 10.7 instead of 12.9 node visits per ray)
    uint32_t trace_queue = 32;                  // MSK_TRACE_QUEUE (at most 64)
    uint32_t trace_split = 2;                   // MSK_TRACE_SPLIT (at least 1)
    size_t trace_pad_lds = 0, shade_pad_lds = 0;     // MSK_TRACE_PAD_LDS_KB, MSK_SHADE_PAD_LDS_KB, in bytes: occupancy experiments only
    const char *dump_rays = nullptr;            // MSK_DUMP_RAYS (measurements only: dump_rays in msk_gpu.hip)
    uint32_t dump_iter = 12, dump_stride = 32;  // MSK_DUMP_ITER, MSK_DUMP_STRIDE (at least 1)
};

inline RenderKnobs read_render_knobs() {
    RenderKnobs k;
    k.regions = env_opt("MSK_REGIONS"); k.region_size = env_opt("MSK_REGION_SIZE");
    k.streams = env_u32("MSK_STREAMS", 4); k.stream_skew = env_u32("MSK_STREAM_SKEW", 10);
    k.host_threads = env_u32("MSK_HOST_THREADS", 1);
    k.sync_group = env_u32("MSK_SYNC_GROUP", 8);
    k.timing_every = std::max(1u, env_u32("MSK_TIMING_EVERY", 1));
    k.sort = env_u32("MSK_SORT", 1) != 0;
    k.camera_cull = env_u32("MSK_CAMERA_CULL", 1) != 0;
    k.force_general_shade = env_u32("MSK_FORCE_GENERAL_SHADE", 0) != 0;
    k.fused = env_u32("MSK_FUSED", 0) != 0; k.fused_hbm = env_u32("MSK_FUSED_HBM", 1) != 0;
    k.fused_iters = std::max(1u, env_u32("MSK_FUSED_ITERS", 16));
    k.fused_tail_pct = env_opt("MSK_FUSED_TAIL_PCT");
    k.trace_refill = getenv("MSK_TRACE_REFILL") ? atoi(getenv("MSK_TRACE_REFILL")) : -1;
    k.trace_quantum = (int) env_u32("MSK_TRACE_QUANTUM", 3);
    k.trace_queue = std::min(64u, env_u32("MSK_TRACE_QUEUE", 32));
    k.trace_split = std::max(1u, env_u32("MSK_TRACE_SPLIT", 2));
    k.trace_pad_lds = (size_t) env_u32("MSK_TRACE_PAD_LDS_KB", 0) * 1024; k.shade_pad_lds = (size_t) env_u32("MSK_SHADE_PAD_LDS_KB", 0) * 1024;
    k.dump_rays = getenv("MSK_DUMP_RAYS");
    k.dump_iter = env_u32("MSK_DUMP_ITER", 12); k.dump_stride = std::max(1u, env_u32("MSK_DUMP_STRIDE", 32));
    return k;
}

// width of the tree for scenes that do not fit LDS: 4 (full-precision boxes) or 8 (quantised boxes); MSK_WIDE_BVH overrides, 0 = binary
#ifndef MSK_WIDE_BVH_DEFAULT
#define MSK_WIDE_BVH_DEFAULT 4
#endif
// Every environment knob of scene creation, read ONCE per msk_gpu_scene_create* call by the calling thread and never kept
// between calls (the tests set knobs between two scenes of one process).
struct SceneKnobs {
    const char *pad_scale = nullptr;            // MSK_PAD_SCALE as text: mskscene::pack parses it, and refuses what is no number in [1e-7, 1e-3]
    bool gpu_build = false;                     // MSK_BVH_BUILD=gpu: the tree is built on the device (msk_lbvh.hip), for scenes that change
                                                // between renders; default: the host's binned-SAH builder (msk_bvh.h), the better tree
    uint32_t bvh_leaf = 2;                      // MSK_BVH_LEAF (1..8): triangles per leaf of the device-built tree.  (The one knob with a second
                                                // reader: the host builder's own default leaf size is not 2, and mskbvh::build, which the
                                                // native checks call without knobs, reads the variable itself for the host-built tree.)
    size_t lds_scene_cap = 48 * 1024;           // MSK_LDS_SCENE_KB, in bytes: a tree with its triangles is staged in LDS up to this size
    uint32_t wide_bvh = MSK_WIDE_BVH_DEFAULT;   // MSK_WIDE_BVH
    bool collapse_optimal = true;               // MSK_COLLAPSE_OPTIMAL
    uint32_t quant_bvh = 2;                     // MSK_QUANT_BVH: 2 half-float child boxes, 1 byte-quantised, 0 full precision
    bool wide_lds = false;                      // MSK_WIDE_LDS (experiment)
    uint32_t stack_cap = 16;                    // MSK_STACK_CAP: entries of a lane's stack that live in LDS, for a tree in HBM
};

inline SceneKnobs read_scene_knobs() {
    SceneKnobs k;
    k.pad_scale = getenv("MSK_PAD_SCALE");
    const char *build_env = getenv("MSK_BVH_BUILD");
    k.gpu_build = build_env && !strcmp(build_env, "gpu");
    k.bvh_leaf = getenv("MSK_BVH_LEAF") ? (uint32_t) std::max(1, std::min(8, atoi(getenv("MSK_BVH_LEAF")))) : 2u;
    k.lds_scene_cap = getenv("MSK_LDS_SCENE_KB") ? (size_t) atoi(getenv("MSK_LDS_SCENE_KB")) * 1024 : 48 * 1024;
    k.wide_bvh = env_u32("MSK_WIDE_BVH", MSK_WIDE_BVH_DEFAULT);
    k.collapse_optimal = env_u32("MSK_COLLAPSE_OPTIMAL", 1) != 0;
    k.quant_bvh = env_u32("MSK_QUANT_BVH", 2);
    k.wide_lds = env_u32("MSK_WIDE_LDS", 0) != 0;
    k.stack_cap = env_u32("MSK_STACK_CAP", 16);
    return k;
}

// Short rays (LDS-resident scene): many small regions, one chunk loop per wave: 8192 x 512 = 4 M path slots (0.6 GB of state;
// measured 16384 / 12288 / 8192 / 6144 regions: 42.7 / 41.7 / 41.2 / 41.6 ms for the bench step — the shading kernel streams the
// whole pool's state every iteration and a smaller pool keeps more of it in the 256 MB Infinity Cache, the traversal kernel
// wants many waves per launch).  Long rays (k_trace_r): 4096 regions of 2048 slots = 8 M, so that lane replacement has a long
// list of rays to keep the lanes busy with.
inline void pool_shape(int trace_mode, uint64_t total_samples, const RenderKnobs &knobs, uint32_t *region_size, uint32_t *n_regions) {
    const bool big = tree_in_hbm(trace_mode);
    // trees in HBM: one traversal wave per region at 5 waves per SIMD = 5120 resident waves; with 4096 regions the four loops'
    // launches never filled the GPU (8192 regions: config-5-class render 173 vs 191 ms, config-3-class 205 vs 227 ms)
    // LDS-resident scenes: 6144 x 1024 (with the state's cache policy in place — msk_kernels.h, MSK_NT — fewer, longer regions
    // win over round 1's 8192 x 512: 36.2 vs 37.0 ms per bench step; 5120 … 8192 x 896 … 1280 are within 1 % of each other)
    uint32_t rs = knobs.region_size >= 0 ? (uint32_t) knobs.region_size : (big ? 2048u : 1024u), nr = knobs.regions >= 0 ? (uint32_t) knobs.regions : (big ? 8192u : 6144u);
    rs = std::max(64u, (rs + 63u) & ~63u);
    while (rs > 256 && total_samples / rs < nr) rs = std::max(256u, rs / 2);       // small jobs: keep the GPU full first
    const uint64_t need = (total_samples + rs - 1) / rs;
    if (need < nr) nr = (uint32_t) std::max<uint64_t>(need, 1);
    nr = (nr + 3u) & ~3u;
    *region_size = rs; *n_regions = nr;
}

struct SceneFacts {
    int trace_mode = 0;
    bool lds_scene = false, lds_tables = false, all_diffuse = true, has_regular = false, has_dielectric = false, cull_ok = false;
    bool has_bitmap = false;      // a `bitmap` texture (ABI v8): the instantiations with the texel lookup run, whatever else the scene holds
    bool has_envmap = false;      // an `envmap` emitter (MSK_EMITTER_ENVMAP): the instantiations with the image lookup and its sampling run
    bool has_delta = false;       // a `point`, `spot` or `directional` emitter or a smooth `conductor` (MSK_EMITTER_POINT / _SPOT / _DIRECTIONAL,
                                  // MSK_BSDF_CONDUCTOR): the instantiations with the
                                  // delta light, the mirror lobe and the `constant` sky's own density run, whatever else the scene holds
    bool has_mask = false;        // a `mask` (msk_mask_desc): the instantiations with the opacity lookup, the null lobe and the `scattered` bit run,
                                  // whatever else the scene holds
    bool has_plastic = false;     // a `plastic` or a `roughplastic` (MSK_BSDF_PLASTIC, MSK_BSDF_ROUGHPLASTIC): the same instantiations run (they carry its two lobes and the per-sample delta mark);
                                  // the scene has mask records of opacity 1 where it holds no mask
    bool has_lens = false;        // a `thinlens` sensor (msk_lens_desc): the instantiations whose new camera samples start on the lens run, whatever
                                  // else the scene holds
    size_t trace_lds_bytes = 0, shade_lds_bytes = 0;
};
// LDS plan of k_shade_gen: the small lookup tables (mesh / BSDF / emitter records, cdf, d65, cie, tabulated spectra), and with
// them, when everything fits, the per-triangle ones (tri_verts, tri_frames).  In float4, from the counts DeviceScene holds.
// (The kernels size what they stage with the same sums: msk_kernels.h, small_tables_float4s and tables_lds_float4s.)
struct TableCounts { uint32_t n_tris = 0, n_meshes = 0, n_bsdf_f4 = 0, n_emitters = 0, cdf_len = 0, n_spectra = 0; };
inline size_t small_bytes(const TableCounts &c) {
    return ((size_t) c.n_meshes + c.n_bsdf_f4 + c.n_emitters * 3 + (c.n_emitters * 95 + 3) / 4 + (c.cdf_len + 3) / 4 + 72 + (c.n_spectra + 3) / 4) * 16;
}
inline size_t table_bytes(const TableCounts &c) { return (size_t) c.n_tris * 6 * 16 + small_bytes(c); }
struct TablePlacement {
    bool lds_tables = false;        // every table in LDS (k_shade_gen<true, ...>)
    size_t staged_bytes = 0;        // what a block stages: all tables, else the small ones if they fit kSmallTablesLimit, else nothing
    size_t shade_lds_bytes = 0;     // + the waves' done-queues
};
inline TablePlacement place_tables(const TableCounts &c) {
    TablePlacement p;
    p.lds_tables = table_bytes(c) <= kLdsTablesLimit;
    // (a scene whose per-triangle tables stay in HBM still stages the small ones)
    p.staged_bytes = p.lds_tables ? table_bytes(c) : small_bytes(c) <= kSmallTablesLimit ? small_bytes(c) : 0;
    p.shade_lds_bytes = p.staged_bytes + kDoneQueueBytes;
    return p;
}

// LDS plan of the traversal kernels: which form of the tree they walk, from where, with how much stack.
struct BinaryTree { uint32_t n_nodes = 0, n_tris = 0; int max_depth = 0; bool root_is_leaf = false; };    // what the builder made (msk_bvh.h)
struct WideTree {                   // what a collapse of it made (msk_bvh.h: collapse4 / collapse8)
    bool ok = false;                // collapse8 refuses a tree whose boxes cannot be quantised conservatively (extents beyond the exponent range)
    int max_depth = 0; uint32_t n_nodes = 0;
    bool has_half = false, has_byte = false;    // 4-wide: the half-float / byte-quantised forms exist (nodes4h / nodes4q are not empty)
};
struct TreePlacement {
    int trace_mode = TRACE_BIN_LDS;
    bool lds_scene = false;
    uint32_t stack_entries = 0;     // DeviceScene::stack_entries: of a lane's stack in LDS ...
    uint32_t stack_total = 0;       // ... and in all; the rest lives in an HBM overflow array (LaneStack)
    size_t trace_lds_bytes = 0;
    size_t binary_stack_bytes = 0;  // the binary tree's whole stack per block (the refusal of a tree too deep for LDS names it)
};
// `collapse(width)` is called at most twice, in the order the forms are tried, and returns the WideTree of that width: the 8-wide
// form may refuse (the 4-wide one is then tried), the quantised 4-wide forms may be missing (the full-precision one is then walked).
template <class Collapse>
inline TreePlacement place_tree(const BinaryTree &t, const SceneKnobs &k, Collapse &&collapse) {
    TreePlacement p;
    // per-lane stack + (when it fits) the whole BVH
    p.stack_entries = (uint32_t) ((t.max_depth + 2 + 3) & ~3);
    p.binary_stack_bytes = (size_t) p.stack_entries * MSK_BLOCK * 4;
    const size_t scene_bytes = (size_t) t.n_nodes * 64 + (size_t) t.n_tris * 96;
    p.lds_scene = scene_bytes <= k.lds_scene_cap && p.binary_stack_bytes + scene_bytes <= kLdsLimit;
    p.trace_lds_bytes = p.binary_stack_bytes + (p.lds_scene ? scene_bytes : 0);
    p.trace_mode = p.lds_scene ? TRACE_BIN_LDS : TRACE_BIN_HBM;
    WideTree w;
    if (!p.lds_scene && k.wide_bvh == 8 && !t.root_is_leaf && (w = collapse(8)).ok) {
        // the tree stays in HBM/L2: eight quantised child boxes per 128-byte line
        p.stack_entries = (uint32_t) ((7 * w.max_depth + 2 + 3) & ~3);     // up to seven pushes per level
        p.trace_mode = TRACE_WIDE8;
    } else if (!p.lds_scene && k.wide_bvh && !t.root_is_leaf) {
        // the tree stays in HBM/L2: walk it four children at a time, one 128-byte line per visit
        w = collapse(4);
        p.stack_entries = (uint32_t) ((3 * w.max_depth + 2 + 3) & ~3);     // up to three pushes per level
        // the walked form (MSK_QUANT_BVH): 2 (default since round 5) 80-byte nodes with half-float child boxes read by v_fma_mix_f32,
        // 1 64-byte nodes with byte-quantised boxes (rounds 3-4), 0 the full-precision 128-byte ones.  Config-5 / config-3 class
        // renders (round 5, same box): 124.7 / 159.5 ms with 2 against 126.9 / 168.3 with 1.
        p.trace_mode = k.quant_bvh == 2 && w.has_half ? TRACE_WIDE4_HALF : k.quant_bvh && w.has_byte ? TRACE_WIDE4_BYTE : TRACE_WIDE4;
    } else if (p.lds_scene && k.wide_lds && !t.root_is_leaf) {
        // experiment knob, off by default: the 4-wide tree staged in LDS (half the dependent LDS round trips per ray).
        // Measured on cbox: trace 12.45 vs 12.34 ms for the binary tree — no gain.
        w = collapse(4);
        p.stack_entries = (uint32_t) ((3 * w.max_depth + 2 + 3) & ~3);
        p.trace_lds_bytes = (size_t) p.stack_entries * MSK_BLOCK * 4 + ((size_t) w.n_nodes * 128 + (size_t) t.n_tris * 96);
        p.trace_mode = TRACE_WIDE4_LDS;
    }
    p.stack_total = p.stack_entries;
    if (tree_in_hbm(p.trace_mode)) {
        // trees in HBM: only the first MSK_STACK_CAP entries of a lane's stack live in LDS, the rest in an HBM overflow
        // array (LaneStack) — any tree depth works within a fixed 16 KB (+ 4 KB of node4_step scratch) of LDS per block, which
        // leaves room for six blocks per CU.  (Measured: the cap does not change the trace time between 8 and 40 entries.)
        p.stack_entries = std::min(p.stack_total, std::max(4u, k.stack_cap & ~3u));
        p.trace_lds_bytes = (size_t) p.stack_entries * MSK_BLOCK * 4 + (size_t) MSK_BLOCK * 16;       // + four words per lane (node4_step)
    }
    return p;
}

struct CallFacts {
    uint32_t region_size = 0;
    uint32_t aov_groups = 0;      // an "aov" render's primary-hit record groups
    bool aov_rgb = false;         // ... and its nested path integrator's RGB record
};

enum TraceFamily : int {
    TRACE_FAMILY_R,        // k_trace_r<mode>: lane replacement, both rays of a slot walked together
    TRACE_FAMILY_Q,        // k_trace_q: the LDS-resident scene's job queues
    TRACE_FAMILY_PLAIN     // k_trace<mode>: the chunk loop
};

enum ShadeKind : int {     // in the order they are tried: a dielectric scene is never diffuse_only, a diffuse_only sweep evaluates no table
    SHADE_DIELECTRIC,      // k_shade_gen_d<lds_tables>;                k_wavefront_d / k_wavefront_h_d
    SHADE_DIFFUSE,         // k_shade_gen<lds_tables, true>;            k_wavefront<true> / k_wavefront_h<true>
    SHADE_REGULAR,         // k_shade_gen<lds_tables, false, true>;     k_wavefront<false, true> / k_wavefront_h<false, true>
    SHADE_GENERAL,         // k_shade_gen<lds_tables, false>;           k_wavefront<false> / k_wavefront_h<false>
    SHADE_BITMAP,          // k_shade_gen_b<lds_tables>;                k_wavefront_b / k_wavefront_h_b.  Tried before the older ones (a scene
                           // with a bitmap runs these whatever else it holds); behind them in the enum, whose older values are indices elsewhere
    SHADE_ENVMAP,          // k_shade_gen_e<lds_tables>;                k_wavefront_e / k_wavefront_h_e.  Tried before those above: a scene with
                           // an `envmap` emitter runs these whatever else it holds (they carry the bitmap lookup and the delta lobes)
    SHADE_DELTA,           // k_shade_gen_p<lds_tables>;                k_wavefront_p / k_wavefront_h_p.  Tried before those above: a scene with a
                           // `point` emitter or a smooth `conductor` runs these whatever else it holds (they carry the envmap lookup as well)
    SHADE_MASK,            // k_shade_gen_m<lds_tables>;                k_wavefront_m / k_wavefront_h_m.  Tried before those above: a scene with a
                           // `mask` runs these whatever else it holds (they carry everything the delta ones do)
    SHADE_LENS             // k_shade_gen_l<lds_tables>;                k_wavefront_l / k_wavefront_h_l.  Tried FIRST: a scene with a `thinlens`
                           // sensor runs these whatever else it holds (they carry everything the mask ones do)
};

struct LaunchPlan {
    // shading: the scene's and the call's flags, and the instantiation they select (shade_kind, also the fused kernels')
    bool lds_tables = false, diffuse_only = false, regular = false, dielectric = false;
    ShadeKind shade_kind = SHADE_GENERAL;
    bool sort_on = false;              // PassParams::sort_scratch: material-sorted shading
    size_t shade_lds_bytes = 0;        // tables + done-queues + the sort's permutation + MSK_SHADE_PAD_LDS_KB
    // traversal
    TraceFamily trace_family = TRACE_FAMILY_PLAIN;
    int trace_mode = 0;
    int refill = 0, max_inner = 3;     // k_trace_r's arguments
    uint32_t queue_refill = 0;         // k_trace_q's
    size_t trace_lds_bytes = 0;        // of the family that runs (k_trace_q: + one bit per slot and wave, from bits_off on)
    size_t bits_off = 0;               // k_trace_q: byte offset of those bits
    uint32_t trace_waves = 1;          // waves per region of the launch's grid
    uint32_t trace_split = 1;          // PassParams::trace_split
    bool lane_refill = false;          // msk_stats::bytes_trace: 16 B per shadow ray instead of 32
    // the fused kernels (k_wavefront*, iterations on the device)
    bool fused_ok = false, fused_h = false, fused_all = false;
    uint32_t fused_iters = 16, fused_tail_pct = 0;
    size_t fused_lds_bytes = 0;
    uint32_t fused_queue_f4 = 0, fused_trace_f4 = 0;       // float4 offsets of the done-queues (after the staged tables) and of the traversal's LDS
    // the loop
    bool cull = false;                 // PassParams::cull
    uint32_t sync_group = 8, timing_every = 1;
};

// The shading family a scene runs, whatever the call: the first feature it holds in the order lens, mask (or plastic, which lives in
// the mask family), delta, envmap, bitmap, dielectric — each family's kernels carry everything the later ones' do.  SHADE_GENERAL: none of them; the wavefront path then
// picks among the three base kinds per call (make_launch_plan), MSK_RNG_PCG_BLOCK runs k_path_serial.
inline ShadeKind shade_family(const SceneFacts &sc) {
    return sc.has_lens ? SHADE_LENS : (sc.has_mask || sc.has_plastic) ? SHADE_MASK : sc.has_delta ? SHADE_DELTA : sc.has_envmap ? SHADE_ENVMAP : sc.has_bitmap ? SHADE_BITMAP :
           sc.has_dielectric ? SHADE_DIELECTRIC : SHADE_GENERAL;
}

inline LaunchPlan make_launch_plan(const SceneFacts &sc, const CallFacts &call, const RenderKnobs &knobs) {
    LaunchPlan p;
    const ShadeKind family = shade_family(sc);
    const bool aov_any = call.aov_rgb || call.aov_groups;
    // camera samples that miss the scene's bounds are finished where they are made (shade_region's regeneration) — unless a miss
    // is more than a record of zeros: an "aov" render's record groups and nested RGB record are written per sample by other code
    p.cull = sc.cull_ok && !aov_any && knobs.camera_cull;
    // (MSK_FORCE_GENERAL_SHADE=1, measurements only: an all-diffuse scene through the general variant — what a per-class diffuse
    // instantiation could save a mixed scene's diffuse chunks)
    // (the AOV RGB record and the validity test over an "aov" render's record groups live in the general shading variant)
    p.lds_tables = sc.lds_tables; p.regular = sc.has_regular; p.dielectric = family != SHADE_GENERAL;      // (the bitmap / envmap / delta / mask / lens instantiations carry the delta lobes)
    p.diffuse_only = sc.all_diffuse && !aov_any && !knobs.force_general_shade;
    p.shade_kind = family != SHADE_GENERAL ? family : p.diffuse_only ? SHADE_DIFFUSE : p.regular ? SHADE_REGULAR : SHADE_GENERAL;
    // material-sorted shading (general variant): LDS for the permutation, 3 bytes per slot of a region and wave (MSK_SORT=0: off)
    const size_t sort_lds = kWavesPerBlock * 3 * call.region_size;
    p.sort_on = !p.diffuse_only && (!sc.all_diffuse || knobs.force_general_shade) && call.region_size <= 4096 && knobs.sort &&
                sc.shade_lds_bytes + sort_lds <= kLdsLimit;
    p.shade_lds_bytes = sc.shade_lds_bytes + (p.sort_on ? sort_lds : 0) + knobs.shade_pad_lds;

    // Lane replacement pays when rays are long (tree in HBM/L2: trace -35 % on the 70 k-triangle scene) and costs when they
    // are short (LDS-resident cbox: +50 %): on by default for trees in HBM only.  MSK_TRACE_REFILL=0 turns it off.
    p.trace_mode = sc.trace_mode;
    p.refill = sc.trace_mode == TRACE_WIDE4_LDS ? 0 : knobs.trace_refill >= 0 ? knobs.trace_refill : (sc.trace_mode == TRACE_BIN_LDS ? 0 : 16);
    p.max_inner = knobs.trace_quantum;
    p.trace_split = sc.trace_mode == TRACE_BIN_LDS ? knobs.trace_split : 1u;
    const size_t lds = sc.trace_lds_bytes + knobs.trace_pad_lds;
    // LDS-resident scenes: k_trace_q (job queues with lane replacement, refill when 32 lanes are idle); MSK_TRACE_QUEUE=0: k_trace<0>
    p.queue_refill = knobs.trace_refill >= 0 ? 0u : knobs.trace_queue;
    p.bits_off = (lds + 15) & ~(size_t) 15;
    const size_t lds_q = p.bits_off + kWavesPerBlock * (call.region_size / 8);       // + one bit per slot and wave
    p.trace_lds_bytes = lds;
    if (p.refill > 0) p.trace_family = TRACE_FAMILY_R;
    else if (sc.trace_mode == TRACE_BIN_LDS && p.queue_refill && sc.lds_scene && lds_q <= kLdsLimit) { p.trace_family = TRACE_FAMILY_Q; p.trace_lds_bytes = lds_q; }
    else p.trace_family = TRACE_FAMILY_PLAIN;
    // k_trace_q and k_trace<0>: trace_split waves per region (LDS-resident scene: no stack overflow array to size).
    // Measured: 2 waves per region -6 % trace on the cbox (twice the waves to balance the tail of a launch), 4 the same.
    p.trace_waves = p.trace_family != TRACE_FAMILY_R && sc.trace_mode == TRACE_BIN_LDS ? p.trace_split : 1u;
    // (a scene in LDS that MSK_TRACE_REFILL forces onto k_trace_r<0> is still counted at 32 B per shadow ray: bench.py and the
    // tests compare msk_stats::bytes_trace between builds)
    p.lane_refill = p.refill > 0 && sc.trace_mode != TRACE_BIN_LDS;

    // k_wavefront (iterations on the device): possible when tables and tree are LDS-resident and everything fits one block's LDS
    // next to each other, and there is no per-iteration AOV kernel.  MSK_FUSED=1: the whole pass; MSK_FUSED_TAIL_PCT=p: from
    // the point where every sample has been started and fewer than p % of the slots are live.
    p.fused_queue_f4 = (uint32_t) ((sc.shade_lds_bytes - kDoneQueueBytes) / 16);
    p.fused_trace_f4 = (uint32_t) (sc.shade_lds_bytes / 16);
    p.fused_lds_bytes = sc.shade_lds_bytes + sc.trace_lds_bytes;
    // ... and k_wavefront_h for the default tree in HBM (trace mode 6): the VERY thin end only (MSK_FUSED_HBM=0: off).  Round 6, same
    // box, config-5 / config-3 class renders: from 10 % live slots on (the LDS-resident scenes' threshold) 117.9 / 137.1 ms against
    // 116.2 / 138.6 without — a wave's own longest rays bound both, and the fused kernel walks them at two waves per SIMD without lane
    // replacement; from 1-3 % on — the ~40 last iterations, whose launches are a few dozen microseconds of latency each —
    // 118.1-118.2 / 143.9-144.2 ms against 119.2 / 146.2 (profiles/r06_ab_fused_hbm.txt): the default, at 2 %.
    p.fused_h = sc.trace_mode == TRACE_WIDE4_HALF && !sc.lds_tables && knobs.fused_hbm;
    p.fused_ok = ((sc.trace_mode == TRACE_BIN_LDS && sc.lds_tables) || p.fused_h) && p.fused_lds_bytes <= kLdsLimit && !call.aov_groups;
    p.fused_all = p.fused_ok && knobs.fused;
    p.fused_iters = knobs.fused_iters;
    p.fused_tail_pct = p.fused_ok ? (knobs.fused_tail_pct >= 0 ? (uint32_t) knobs.fused_tail_pct : (p.fused_h ? 2u : 10u)) : 0u;

    p.sync_group = knobs.sync_group; p.timing_every = knobs.timing_every;
    return p;
}

// ---- the "direct" integrator (msk_direct.h: k_direct<form>) -------------------------------------------------------------------------
// One lane owns one camera sample through its 1 + N + M rays, a wave owns `records_per_wave` consecutive records of the pass, a
// launch `records_per_launch` of them.  The form follows the scene's tree: the binary tree staged in LDS beside the shading tables,
// the half-float 4-wide tree in HBM (the default for a tree that stays there), or — every other trace mode — the binary tree in
// HBM, which every scene has (as k_path_serial walks it).  The tables a block stages are the scene's own placement (all of them,
// the small ones, or none) unless they do not fit beside the tree and the stacks: then they are read from HBM / L2.
constexpr uint32_t kDirectMaxSamples = 4096;                       // light_samples and bsdf_samples, each
constexpr uint64_t kDirectRaysPerLaunch = 1ull << 26;              // a launch traces about this many rays ...
constexpr uint64_t kDirectMinWaves = 2048;                         // ... but is never cut below two waves per SIMD of 256 CUs
constexpr uint32_t kDirectWavesPerLaunch = 8192;                   // records_per_wave aims at this many waves per launch,
constexpr uint32_t kDirectMaxRecordsPerWave = 1024;                // within [MSK_WAVE, this]
struct DirectPlan {
    int form = TRACE_BIN_LDS;          // k_direct's MODE: TRACE_BIN_LDS, TRACE_WIDE4_HALF or TRACE_BIN_HBM
    uint32_t tables_mode = 0;          // what a block stages: 0 nothing, 1 the small tables, 2 all tables
    uint32_t stack_f4 = 0;             // float4 offset of the traversal stacks in the block's LDS (behind the staged tables)
    uint32_t stack_entries = 0;        // of a lane's stack in LDS ...
    uint32_t ovf_entries = 0;          // ... and in the HBM overflow array (LaneStack)
    size_t lds_bytes = 0;
    uint32_t rays_per_sample = 0;      // 1 + N + M: the most a sample can trace
    uint32_t records_per_wave = MSK_WAVE;
    uint64_t records_per_launch = 0;   // a multiple of records_per_wave
    uint64_t n_launches = 0;           // of a pass of `pass_records` records
    uint32_t grid_blocks(uint64_t records) const {
        const uint64_t waves = (records + records_per_wave - 1) / records_per_wave;
        return (uint32_t) ((waves + kWavesPerBlock - 1) / kWavesPerBlock);
    }
};
// dev_stack_entries / dev_stack_total: DeviceScene's, of the tree the scene's trace mode walks; bvh_depth: the binary tree's
inline DirectPlan make_direct_plan(const SceneFacts &sc, uint32_t dev_stack_entries, uint32_t dev_stack_total, int bvh_depth,
                                   uint32_t light_samples, uint32_t bsdf_samples, uint64_t pass_records) {
    DirectPlan p;
    size_t staged = sc.shade_lds_bytes >= kDoneQueueBytes ? sc.shade_lds_bytes - kDoneQueueBytes : 0;
    size_t trace_bytes;
    if (sc.trace_mode == TRACE_BIN_LDS) {
        p.form = TRACE_BIN_LDS;
        p.stack_entries = dev_stack_entries; p.ovf_entries = 0;
        trace_bytes = sc.trace_lds_bytes;                                       // the whole stack + tree + triangles
    } else {
        uint32_t total = dev_stack_total;
        p.form = TRACE_WIDE4_HALF; p.stack_entries = dev_stack_entries;
        if (sc.trace_mode != TRACE_WIDE4_HALF) {                                // the binary tree in HBM: depth + 2 entries
            p.form = TRACE_BIN_HBM;
            total = (uint32_t) bvh_depth + 2u;
            p.stack_entries = std::max(4u, std::min(dev_stack_entries, (total + 3u) & ~3u));
        }
        p.ovf_entries = total > p.stack_entries ? total - p.stack_entries : 0u;
        trace_bytes = (size_t) p.stack_entries * MSK_BLOCK * 4 + (size_t) MSK_BLOCK * 16;      // + four words per lane (node4h_step)
    }
    if (staged + trace_bytes > kLdsLimit) staged = 0;
    p.tables_mode = staged == 0 ? 0u : sc.lds_tables ? 2u : 1u;
    p.stack_f4 = (uint32_t) (staged / 16);
    p.lds_bytes = staged + trace_bytes;
    p.rays_per_sample = 1u + light_samples + bsdf_samples;
    uint64_t per_launch = std::max<uint64_t>(kDirectRaysPerLaunch / p.rays_per_sample, kDirectMinWaves * MSK_WAVE);
    per_launch = std::min(per_launch, std::max<uint64_t>(pass_records, 1));
    const uint64_t per_wave = ((per_launch + kDirectWavesPerLaunch - 1) / kDirectWavesPerLaunch + MSK_WAVE - 1) / MSK_WAVE * MSK_WAVE;
    p.records_per_wave = (uint32_t) std::min<uint64_t>(kDirectMaxRecordsPerWave, std::max<uint64_t>(MSK_WAVE, per_wave));
    p.records_per_launch = (per_launch + p.records_per_wave - 1) / p.records_per_wave * p.records_per_wave;
    p.n_launches = (pass_records + p.records_per_launch - 1) / p.records_per_launch;
    return p;
}

// The static, interleaved partition of a pass's samples over the regions (RegionCtl): chunks of 64 samples dealt round robin,
// the last chunk partial.  The regions' initial records and what a part of the pool expects to finish both come from here.
inline unsigned long long region_share(unsigned long long total, uint32_t n_regions, uint32_t r) {
    const unsigned long long n_chunks = (total + 63) / 64;
    const unsigned long long mine = n_chunks > r ? (n_chunks - r + n_regions - 1) / n_regions : 0;
    unsigned long long n = mine * 64;
    if (mine && (mine - 1) * n_regions + r == n_chunks - 1) n -= n_chunks * 64 - total;   // partial last chunk
    return n;
}

// Cuts the pool's regions into n_parts consecutive parts; part k is [out[k], out[k + 1]).  Parts of slightly different sizes:
// equal parts can fall into step (all launches starting and draining together, which is one big launch again; measured as a
// bimodal 48 / 52 ms), unequal ones keep sliding past each other.  skew_pct: relative size step between neighbouring parts.
inline std::vector<uint32_t> part_ranges(uint32_t n_regions, uint32_t n_parts, uint32_t skew_pct) {
    const double skew = skew_pct / 100.0;
    std::vector<double> cum(n_parts + 1, 0.0);
    for (uint32_t k = 0; k < n_parts; ++k) cum[k + 1] = cum[k] + 1.0 + skew * ((double) (n_parts - 1) / 2.0 - k);
    std::vector<uint32_t> out(n_parts + 1, n_regions);
    for (uint32_t k = 0; k < n_parts; ++k) out[k] = (uint32_t) (n_regions * (cum[k] / cum[n_parts]));
    return out;
}

}  // namespace mskplan
