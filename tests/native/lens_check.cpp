// lens_check.cpp — the `thinlens` sensor's host side on a CPU, for tests/test_thinlens.py.  Stand-alone; built with and without
// -fsanitize=address,undefined.
//   lens_check                  csrc/msk_lens_tables.h: every bad msk_lens_desc is refused with MSK_ERR_INVALID_ARG and a text that names
//                               its field, every good one passes; add_lens_tables gives a scene without masks the mask records of the
//                               constant opacity 1 and leaves a scene with masks alone.  Prints "ok <checks>".
//   lens_check layout           sizes and offsets of msk_lens_desc and msk_scene_lens, one line of numbers (the test compares them
//                               with abi.py's ctypes structures).
//   lens_check exports <lib>    dlopen(<lib>) exports msk_gpu_scene_create_lens and msk_gpu_camera_sample.  Prints "exports 2".
//   lens_check plan             csrc/msk_plan.h over the cross product of mask_tables_check.cpp with has_mask added (knobs from the
//                               environment): with SceneFacts::has_lens the plan names SHADE_LENS whatever else the scene holds and every
//                               other field is what the same facts give with has_mask instead; without it the plan names what the
//                               ladder named before.  Prints "cases N".
// Returns 0, or prints the first failure and returns 1.
#include "../../misaki-render_amd/csrc/msk_lens_tables.h"
#include "../../misaki-render_amd/csrc/msk_plan.h"

#include <dlfcn.h>

#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

static int n_checks = 0;
#define CHECK(cond, ...) do { ++n_checks; if (!(cond)) { std::printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); return 1; } } while (0)

struct Scene {
    std::vector<msk_mesh_desc> meshes;
    std::vector<msk_bsdf_desc> bsdfs;
    std::vector<msk_emitter_desc> emitters;
    std::vector<float> vertices;
    std::vector<uint32_t> faces;
    float cie[3 * MSK_CIE_SAMPLES], d65[MSK_CIE_SAMPLES];
    msk_scene_desc d;
};

static msk_bsdf_desc diffuse(float c) {
    msk_bsdf_desc b;
    std::memset(&b, 0, sizeof b);
    b.type = MSK_BSDF_DIFFUSE; b.back_bsdf = -1;
    b.reflectance[0] = c; b.reflectance[1] = 0.5f; b.reflectance[2] = -0.75f; b.reflectance_scale = 1.f;
    const msk_spectrum_desc one = {{0.f, 0.f, INFINITY}, 1.f, 0u};
    b.eta = b.k = b.specular_reflectance = b.specular_transmittance = one;
    b.ior_eta = b.ior_inv_eta = 1.f;
    return b;
}
static void quad(Scene &s, float y, int32_t bsdf, int32_t em) {
    msk_mesh_desc m;
    std::memset(&m, 0, sizeof m);
    m.first_vertex = (uint32_t) (s.vertices.size() / 8); m.vertex_count = 4;
    m.first_face = (uint32_t) (s.faces.size() / 3); m.face_count = 2;
    m.bsdf_id = bsdf; m.emitter_id = em;
    const float p[4][2] = {{0, 0}, {3, 0}, {3, 2}, {0, 2}};
    for (int k = 0; k < 4; ++k) { const float v[8] = {p[k][0], y, p[k][1], 0.f, 1.f, 0.f, 0.f, 0.f}; s.vertices.insert(s.vertices.end(), v, v + 8); }
    const uint32_t f[6] = {0, 2, 1, 0, 3, 2};
    s.faces.insert(s.faces.end(), f, f + 6);
    s.meshes.push_back(m);
}
// two diffuse quads, the second an area light
static void make(Scene &s) {
    std::memset(&s.d, 0, sizeof s.d);
    s.d.abi_version = MSK_ABI_VERSION;
    for (int i = 0; i < 3 * MSK_CIE_SAMPLES; ++i) s.cie[i] = 0.0078125f * (float) ((i * 37) % 101);
    for (int i = 0; i < MSK_CIE_SAMPLES; ++i) s.d65[i] = 40.f + 0.75f * (float) ((i * 11) % 64);
    for (int k = 0; k < 4; ++k) { s.d.camera.sample_to_camera[k * 5] = 1.f; s.d.camera.to_world[k * 5] = 1.f; }
    s.d.camera.near_clip = 0.01f; s.d.camera.far_clip = 100.f;
    s.d.film.width = 16; s.d.film.height = 8; s.d.film.filter_radius = 0.5f;
    for (int i = 0; i < MSK_FILTER_RESOLUTION; ++i) s.d.film.filter_lut[i] = 1.f;
    msk_emitter_desc e;
    std::memset(&e, 0, sizeof e);
    e.type = MSK_EMITTER_AREA; e.mesh_id = 1; e.radiance[0] = 0.5f; e.radiance[1] = -0.25f; e.radiance[2] = 2.f; e.d65_scale = 0.015625f;
    s.emitters.push_back(e);
    quad(s, 0.f, 0, -1); quad(s, 1.f, 1, 0);
    s.bsdfs = {diffuse(0.25f), diffuse(0.f)};
    s.d.n_meshes = (uint32_t) s.meshes.size(); s.d.meshes = s.meshes.data();
    s.d.n_bsdfs = (uint32_t) s.bsdfs.size(); s.d.bsdfs = s.bsdfs.data();
    s.d.n_emitters = (uint32_t) s.emitters.size(); s.d.emitters = s.emitters.data();
    s.d.n_vertices = (uint32_t) (s.vertices.size() / 8); s.d.vertices = s.vertices.data();
    s.d.n_faces = (uint32_t) (s.faces.size() / 3); s.d.faces = s.faces.data();
    s.d.cie1931_xyz = s.cie; s.d.d65 = s.d65;
}

static int refused(float radius, float focus, const char *field) {
    const msk_lens_desc l = {radius, focus};
    std::string msg;
    const int rc = mskscene::check_lens(&l, &msg);
    CHECK(rc == MSK_ERR_INVALID_ARG, "{%g, %g}: code %d, message \"%s\"", (double) radius, (double) focus, rc, msg.c_str());
    CHECK(msg.find("msk_lens_desc") != std::string::npos && msg.find(field) != std::string::npos, "{%g, %g}: \"%s\" does not name %s", (double) radius, (double) focus,
          msg.c_str(), field);
    return 0;
}
static int accepted(float radius, float focus) {
    const msk_lens_desc l = {radius, focus};
    std::string msg = "untouched";
    CHECK(mskscene::check_lens(&l, &msg) == MSK_OK && msg == "untouched", "{%g, %g}: \"%s\"", (double) radius, (double) focus, msg.c_str());
    return 0;
}

static int validation_check() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float tiny = std::numeric_limits<float>::denorm_min(), big = std::numeric_limits<float>::max();
    std::string msg;
    CHECK(mskscene::check_lens(nullptr, &msg) == MSK_OK && msg.empty(), "no lens is no refusal");
    // aperture_radius: negative, NaN, infinite
    for (float r : {-1.f, -tiny, -big, -inf, inf, nan, -nan}) if (refused(r, 5.f, "aperture_radius")) return 1;
    // focus_distance: not finite, not greater than 0
    for (float f : {0.f, -0.f, -1.f, -tiny, -big, -inf, inf, nan, -nan}) if (refused(0.25f, f, "focus_distance")) return 1;
    // both bad: the radius is named first
    if (refused(-1.f, -1.f, "aperture_radius")) return 1;
    // the limits themselves are taken
    for (float r : {0.f, -0.f, tiny, 0.25f, big}) for (float f : {tiny, 1.f, 1e4f, big}) if (accepted(r, f)) return 1;

    // ---- the tables of a scene with a lens
    Scene s; make(s);
    mskscene::HostTables a, b;
    CHECK(mskscene::pack(&s.d, nullptr, nullptr, &a, &msg) == MSK_OK, "pack: %s", msg.c_str());
    b = a;
    CHECK(a.all_diffuse && !a.has_mask && a.mask_base == 0, "the plain scene's flags");
    mskscene::add_lens_tables(&s.d, &b);
    CHECK(!b.all_diffuse && !b.has_mask, "flags: general shading, and still no mask of the scene's own");
    CHECK(b.mask_base == a.n_bsdf_f4 && b.n_bsdf_f4 == a.n_bsdf_f4 + 3u * s.d.n_bsdfs && b.bsdfs.size() == (size_t) b.n_bsdf_f4 * 4, "three float4 per BSDF entry, appended");
    CHECK(!std::memcmp(a.bsdfs.data(), b.bsdfs.data(), a.bsdfs.size() * 4), "the older records keep their bytes");
    for (uint32_t k = 0; k < s.d.n_bsdfs; ++k) {
        const float *o = &b.bsdfs[((size_t) b.mask_base + 3u * k) * 4];
        for (int i = 0; i < 12; ++i) CHECK(i == 5 ? o[i] == 1.f : (o[i] == 0.f && !std::signbit(o[i])), "entry %u word %d: the constant opacity 1, filter 0", k, i);
    }
    // ... which is, byte for byte, what the packer writes for the same scene with one constant mask of opacity 1
    msk_mask_desc one;
    std::memset(&one, 0, sizeof one);
    one.bsdf = 0; one.filter = 0; one.opacity = 1.f;
    mskscene::HostTables m;
    CHECK(mskscene::pack(&s.d, nullptr, nullptr, &m, &msg, 1, &one) == MSK_OK && m.has_mask, "pack with a mask: %s", msg.c_str());
    CHECK(m.mask_base == b.mask_base && m.n_bsdf_f4 == b.n_bsdf_f4 && m.bsdfs.size() == b.bsdfs.size() && !std::memcmp(m.bsdfs.data(), b.bsdfs.data(), m.bsdfs.size() * 4),
          "the records of an opacity-1 mask");
    // a scene with masks keeps its own records
    mskscene::HostTables m2 = m;
    mskscene::add_lens_tables(&s.d, &m2);
    CHECK(m2.has_mask && m2.n_bsdf_f4 == m.n_bsdf_f4 && m2.bsdfs.size() == m.bsdfs.size() && !std::memcmp(m2.bsdfs.data(), m.bsdfs.data(), m.bsdfs.size() * 4) && !m2.all_diffuse, "a scene with masks is left alone");
    std::printf("ok %d\n", n_checks);
    return 0;
}

static int layout_check() {
    static_assert(sizeof(msk_lens_desc) == 8 && offsetof(msk_lens_desc, aperture_radius) == 0 && offsetof(msk_lens_desc, focus_distance) == 4, "msk_lens_desc layout");
    static_assert(sizeof(msk_scene_lens) == sizeof(msk_scene_lights) + sizeof(void *) && offsetof(msk_scene_lens, lights) == 0 &&
                      offsetof(msk_scene_lens, lens) == sizeof(msk_scene_lights), "msk_scene_lens layout");
    static_assert(MSK_ABI_VERSION == 8, "the ABI version stays");
    std::printf("%zu %zu %zu %zu %zu %zu %zu %d\n", sizeof(msk_lens_desc), offsetof(msk_lens_desc, aperture_radius), offsetof(msk_lens_desc, focus_distance),
                sizeof(msk_scene_lens), offsetof(msk_scene_lens, lights), offsetof(msk_scene_lens, lens), sizeof(msk_scene_lights), MSK_ABI_VERSION);
    return 0;
}

static int exports_check(const char *path) {
    void *h = dlopen(path, RTLD_NOW | RTLD_LOCAL);
    if (!h) { std::printf("dlopen(%s): %s\n", path, dlerror()); return 1; }
    int n = 0;
    for (const char *name : {"msk_gpu_scene_create_lens", "msk_gpu_camera_sample"}) {
        if (!dlsym(h, name)) { std::printf("%s does not export %s\n", path, name); return 1; }
        ++n;
    }
    std::printf("exports %d\n", n);
    return 0;
}

static bool same_but_kind(const mskplan::LaunchPlan &a, const mskplan::LaunchPlan &b) {
    return a.lds_tables == b.lds_tables && a.diffuse_only == b.diffuse_only && a.regular == b.regular && a.dielectric == b.dielectric && a.sort_on == b.sort_on &&
           a.shade_lds_bytes == b.shade_lds_bytes && a.trace_family == b.trace_family && a.trace_mode == b.trace_mode && a.refill == b.refill && a.max_inner == b.max_inner &&
           a.queue_refill == b.queue_refill && a.trace_lds_bytes == b.trace_lds_bytes && a.bits_off == b.bits_off && a.trace_waves == b.trace_waves &&
           a.trace_split == b.trace_split && a.lane_refill == b.lane_refill && a.fused_ok == b.fused_ok && a.fused_h == b.fused_h && a.fused_all == b.fused_all &&
           a.fused_iters == b.fused_iters && a.fused_tail_pct == b.fused_tail_pct && a.fused_lds_bytes == b.fused_lds_bytes && a.fused_queue_f4 == b.fused_queue_f4 &&
           a.fused_trace_f4 == b.fused_trace_f4 && a.cull == b.cull && a.sync_group == b.sync_group && a.timing_every == b.timing_every;
}

static int plan_check() {
    using namespace mskplan;
    static_assert(SHADE_DIELECTRIC == 0 && SHADE_DIFFUSE == 1 && SHADE_REGULAR == 2 && SHADE_GENERAL == 3 && SHADE_BITMAP == 4 && SHADE_ENVMAP == 5 &&
                      SHADE_DELTA == 6 && SHADE_MASK == 7 && SHADE_LENS == 8, "SHADE_LENS is appended: the older values index name tables");
    if (SceneFacts().has_lens) { std::printf("has_lens must default to false\n"); return 1; }
    const RenderKnobs knobs = read_render_knobs();
    static const size_t lds[7][2] = {{24576, 8192}, {53248, 8192}, {53264, 8192}, {24576, 65024}, {24576, 65040}, {24576, 40960}, {24576, 40976}};
    static const uint32_t region_sizes[4] = {256, 1024, 2048, 8192};
    unsigned long n = 0;
    for (int mode = 0; mode <= 6; ++mode)
        for (int flags = 0; flags < 512; ++flags)
            for (int aov = 0; aov < 4; ++aov)
                for (uint32_t rs : region_sizes)
                    for (const auto &b : lds) {
                        SceneFacts s;
                        s.trace_mode = mode; s.lds_scene = mode == TRACE_BIN_LDS || mode == TRACE_WIDE4_LDS;
                        s.lds_tables = flags & 1; s.all_diffuse = flags & 2; s.has_regular = flags & 4; s.has_dielectric = flags & 8; s.cull_ok = flags & 16;
                        s.has_bitmap = flags & 32; s.has_envmap = flags & 64; s.has_delta = flags & 128; s.has_mask = flags & 256;
                        s.shade_lds_bytes = b[0]; s.trace_lds_bytes = b[1];
                        CallFacts c;
                        c.region_size = rs; c.aov_groups = (aov & 1) ? 2u : 0u; c.aov_rgb = (aov & 2) != 0;
                        // the facts scene creation states for a scene with a lens: never all_diffuse (msk_lens_tables.h)
                        SceneFacts sl = s, sm = s;
                        sl.has_lens = true; sl.all_diffuse = false;
                        sm.has_mask = true; sm.all_diffuse = false;
                        const LaunchPlan p = make_launch_plan(s, c, knobs), l = make_launch_plan(sl, c, knobs), m = make_launch_plan(sm, c, knobs);
                        const char *bad = nullptr;
                        if (l.shade_kind != SHADE_LENS) bad = "shade_kind (must be SHADE_LENS)";
                        else if (m.shade_kind != SHADE_MASK) bad = "shade_kind of the comparison plan";
                        else if (!same_but_kind(l, m)) bad = "a field other than shade_kind differs from the plan of the scene with a mask";
                        else if (l.diffuse_only || !l.dielectric) bad = "the lens kernels are general ones with the delta lobes";
                        else if (p.shade_kind == SHADE_LENS) bad = "SHADE_LENS without a lens";
                        const ShadeKind before = s.has_mask ? SHADE_MASK : s.has_delta ? SHADE_DELTA : s.has_envmap ? SHADE_ENVMAP : s.has_bitmap ? SHADE_BITMAP : p.dielectric ? SHADE_DIELECTRIC :
                                                 p.diffuse_only ? SHADE_DIFFUSE : p.regular ? SHADE_REGULAR : SHADE_GENERAL;
                        if (!bad && p.shade_kind != before) bad = "a scene without a lens does not plan what it planned before";
                        if (!bad && p.dielectric != (s.has_dielectric || s.has_bitmap || s.has_envmap || s.has_delta || s.has_mask)) bad = "dielectric of a scene without a lens";
                        if (bad) { std::printf("%s: mode %d flags %d aov %d region_size %u lds %zu %zu\n", bad, mode, flags, aov, rs, b[0], b[1]); return 1; }
                        ++n;
                    }
    std::printf("cases %lu\n", n);
    return 0;
}

int main(int argc, char **argv) {
    const std::string what = argc > 1 ? argv[1] : "";
    if (what == "plan") return plan_check();
    if (what == "layout") return layout_check();
    if (what == "exports") return argc > 2 ? exports_check(argv[2]) : 1;
    return validation_check();
}
