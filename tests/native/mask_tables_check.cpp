// mask_tables_check.cpp — the `mask` part of scene creation's host side on a CPU, for tests/test_mask_bsdf.py: what
// csrc/msk_scene_tables.h (through msk_mask_tables.h) packs for msk_mask_desc (layout), every refusal, that a scene without masks packs to the bytes it had
// without the argument, and that msk_plan.h's byte sums follow the grown BSDF table.  Stand-alone; built with and without
// -fsanitize=address,undefined.  Prints "ok <checks>" and returns 0, or the first failure and 1.
//   mask_tables_check plan      csrc/msk_plan.h over the cross product of launch_plan_delta_check.cpp with has_delta added (knobs from
//                               the environment): with SceneFacts::has_mask the plan names SHADE_MASK whatever else the scene holds and
//                               every other field is what the same facts give with has_mask = false and has_dielectric = true (nothing is
//                               withheld); without it the plan is, field for field, what the facts gave before.  Prints "cases N".
#include "../../misaki-render_amd/csrc/msk_scene_tables.h"
#include "../../misaki-render_amd/csrc/msk_plan.h"

#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

static int n_checks = 0;
#define CHECK(cond, ...) do { ++n_checks; if (!(cond)) { std::printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); return 1; } } while (0)

struct Scene {
    std::vector<msk_mesh_desc> meshes;
    std::vector<msk_bsdf_desc> bsdfs;
    std::vector<msk_emitter_desc> emitters;
    std::vector<msk_texture_desc> textures;
    std::vector<float> vertices, texels;
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
    m.bsdf_id = bsdf; m.emitter_id = em; m.has_texcoords = 1;
    const float p[4][2] = {{0, 0}, {1, 0}, {1, 1}, {0, 1}};
    for (int k = 0; k < 4; ++k) { const float v[8] = {p[k][0], y, p[k][1], 0.f, 1.f, 0.f, p[k][0], p[k][1]}; s.vertices.insert(s.vertices.end(), v, v + 8); }
    const uint32_t f[6] = {0, 2, 1, 0, 3, 2};
    s.faces.insert(s.faces.end(), f, f + 6);
    s.meshes.push_back(m);
}
// two quads, three BSDF entries (the last unreferenced), one area emitter; with_bitmap: a 2 x 1 bitmap reflectance on entry 0
static void make(Scene &s, bool with_bitmap) {
    std::memset(&s.d, 0, sizeof s.d);
    s.d.abi_version = MSK_ABI_VERSION;
    for (int i = 0; i < 3 * MSK_CIE_SAMPLES; ++i) s.cie[i] = 0.0078125f * (float) ((i * 37) % 101);
    for (int i = 0; i < MSK_CIE_SAMPLES; ++i) s.d65[i] = 40.f + 0.75f * (float) ((i * 11) % 64);
    for (int k = 0; k < 4; ++k) { s.d.camera.sample_to_camera[k * 5] = 1.f; s.d.camera.to_world[k * 5] = 1.f; }
    s.d.camera.near_clip = 0.01f; s.d.camera.far_clip = 100.f;
    s.d.film.width = 16; s.d.film.height = 8; s.d.film.filter_radius = 0.5f;
    for (int i = 0; i < MSK_FILTER_RESOLUTION; ++i) s.d.film.filter_lut[i] = 1.f;
    quad(s, 0.f, 0, -1); quad(s, 1.f, 1, 0);
    s.bsdfs = {diffuse(0.25f), diffuse(0.f), diffuse(1.f)};
    msk_emitter_desc e;
    std::memset(&e, 0, sizeof e);
    e.type = MSK_EMITTER_AREA; e.mesh_id = 1; e.radiance[2] = 2.f; e.d65_scale = 0.015625f;
    s.emitters.push_back(e);
    if (with_bitmap) {
        msk_texture_desc t;
        std::memset(&t, 0, sizeof t);
        t.type = MSK_TEXTURE_BITMAP; t.width = 2; t.height = 1; t.to_uv[0] = 1.f; t.to_uv[4] = 1.f;
        s.textures.push_back(t);
        for (int i = 0; i < 6; ++i) s.texels.push_back(0.125f * (float) i);
        s.bsdfs[0].reflectance_texture = 1;
    }
    s.d.n_meshes = (uint32_t) s.meshes.size(); s.d.meshes = s.meshes.data();
    s.d.n_bsdfs = (uint32_t) s.bsdfs.size(); s.d.bsdfs = s.bsdfs.data();
    s.d.n_emitters = 1; s.d.emitters = s.emitters.data();
    s.d.n_vertices = (uint32_t) (s.vertices.size() / 8); s.d.vertices = s.vertices.data();
    s.d.n_faces = (uint32_t) (s.faces.size() / 3); s.d.faces = s.faces.data();
    s.d.n_textures = (uint32_t) s.textures.size(); s.d.textures = s.textures.empty() ? nullptr : s.textures.data();
    s.d.n_texels = (uint32_t) (s.texels.size() / 3); s.d.texels = s.texels.empty() ? nullptr : s.texels.data();
    s.d.cie1931_xyz = s.cie; s.d.d65 = s.d65;
}
static msk_mask_desc constant_mask(uint32_t bsdf, float a) {
    msk_mask_desc m;
    std::memset(&m, 0, sizeof m);
    m.bsdf = bsdf; m.opacity = a; m.filter = 0;
    return m;
}
static msk_mask_desc image_mask(uint32_t bsdf, int filter, uint32_t w, uint32_t h, const float *values) {
    msk_mask_desc m = constant_mask(bsdf, 0.f);
    m.filter = filter; m.width = w; m.height = h; m.values = values;
    const float to_uv[6] = {4.f, 0.5f, 0.125f, -0.25f, 3.f, 0.75f};
    std::memcpy(m.to_uv, to_uv, sizeof to_uv);
    return m;
}
static uint32_t word(const std::vector<float> &v, size_t i) { uint32_t w; std::memcpy(&w, &v[i], 4); return w; }
static bool same(const std::vector<float> &a, const std::vector<float> &b) { return a.size() == b.size() && (a.empty() || !std::memcmp(a.data(), b.data(), a.size() * 4)); }

static int refusal(const char *name, uint32_t n, const msk_mask_desc *ptr, const char *words, int code = MSK_ERR_INVALID_ARG) {
    Scene s; make(s, false);
    mskscene::HostTables t; std::string msg;
    const int rc = mskscene::pack(&s.d, nullptr, nullptr, &t, &msg, n, ptr);
    CHECK(rc == code, "%s: code %d, message \"%s\"", name, rc, msg.c_str());
    CHECK(msg.find(words) != std::string::npos, "%s: \"%s\" does not say \"%s\"", name, msg.c_str(), words);
    CHECK(msg.find("mask") != std::string::npos, "%s: \"%s\" does not name the mask", name, msg.c_str());
    return 0;
}

#define FIELDS(X) X(lds_tables) X(diffuse_only) X(regular) X(dielectric) X(sort_on) X(shade_lds_bytes) X(trace_family) X(trace_mode) X(refill)      \
    X(max_inner) X(queue_refill) X(trace_lds_bytes) X(bits_off) X(trace_waves) X(trace_split) X(lane_refill) X(fused_ok) X(fused_h) X(fused_all) \
    X(fused_iters) X(fused_tail_pct) X(fused_lds_bytes) X(fused_queue_f4) X(fused_trace_f4) X(cull) X(sync_group) X(timing_every)
static int plan_check() {
    using namespace mskplan;
    static_assert(SHADE_DIELECTRIC == 0 && SHADE_DIFFUSE == 1 && SHADE_REGULAR == 2 && SHADE_GENERAL == 3 && SHADE_BITMAP == 4 && SHADE_ENVMAP == 5 &&
                      SHADE_DELTA == 6 && SHADE_MASK == 7, "SHADE_MASK is appended: the older values index name tables");
    const RenderKnobs knobs = read_render_knobs();
    static const size_t lds[7][2] = {{24576, 8192}, {53248, 8192}, {53264, 8192}, {24576, 65024}, {24576, 65040}, {24576, 40960}, {24576, 40976}};
    static const uint32_t region_sizes[4] = {256, 1024, 2048, 8192};
    if (SceneFacts().has_mask) { std::printf("has_mask must default to false\n"); return 1; }
    unsigned long n = 0;
    for (int mode = 0; mode <= 6; ++mode)
        for (int flags = 0; flags < 256; ++flags)
            for (int aov = 0; aov < 4; ++aov)
                for (uint32_t rs : region_sizes)
                    for (const auto &l : lds) {
                        SceneFacts s;
                        s.trace_mode = mode; s.lds_scene = mode == TRACE_BIN_LDS || mode == TRACE_WIDE4_LDS;
                        s.lds_tables = flags & 1; s.all_diffuse = flags & 2; s.has_regular = flags & 4; s.has_dielectric = flags & 8; s.cull_ok = flags & 16;
                        s.has_bitmap = flags & 32; s.has_envmap = flags & 64; s.has_delta = flags & 128;
                        s.shade_lds_bytes = l[0]; s.trace_lds_bytes = l[1];
                        CallFacts c;
                        c.region_size = rs; c.aov_groups = (aov & 1) ? 2u : 0u; c.aov_rgb = (aov & 2) != 0;
                        SceneFacts sm = s, sd = s;
                        sm.has_mask = true;
                        sd.has_bitmap = false; sd.has_envmap = false; sd.has_delta = false; sd.has_dielectric = true;
                        const LaunchPlan e = make_launch_plan(sm, c, knobs), d = make_launch_plan(sd, c, knobs), p = make_launch_plan(s, c, knobs);
                        const char *bad = nullptr;
                        if (e.shade_kind != SHADE_MASK) bad = "shade_kind (must be SHADE_MASK)";
                        if (d.shade_kind != SHADE_DIELECTRIC) bad = "shade_kind of the comparison plan";
                        if (p.shade_kind == SHADE_MASK) bad = "SHADE_MASK without a mask";
                        const ShadeKind before = s.has_delta ? SHADE_DELTA : s.has_envmap ? SHADE_ENVMAP : s.has_bitmap ? SHADE_BITMAP : p.dielectric ? SHADE_DIELECTRIC :
                                                 p.diffuse_only ? SHADE_DIFFUSE : p.regular ? SHADE_REGULAR : SHADE_GENERAL;
                        if (p.shade_kind != before) bad = "a scene without masks does not plan what it planned before";
                        if (p.dielectric != (s.has_dielectric || s.has_bitmap || s.has_envmap || s.has_delta)) bad = "dielectric of a scene without masks";
#define X(f) if (!(e.f == d.f)) bad = #f;
                        FIELDS(X)
#undef X
                        if (bad) { std::printf("mismatch in %s: mode %d flags %d aov %d region_size %u lds %zu %zu\n", bad, mode, flags, aov, rs, l[0], l[1]); return 1; }
                        ++n;
                    }
    std::printf("cases %lu\n", n);
    return 0;
}

int main(int argc, char **argv) {
    if (argc > 1 && std::string(argv[1]) == "plan") return plan_check();
    static_assert(sizeof(msk_mask_desc) == 56 && offsetof(msk_mask_desc, values) == 48, "msk_mask_desc layout");
    static_assert(sizeof(msk_scene_masks) == sizeof(msk_scene_ext) + 16, "msk_scene_masks layout");
    // ---- a scene without masks packs to the bytes it had without the argument, with and without a bitmap
    for (int bm = 0; bm < 2; ++bm) {
        Scene s; make(s, bm);
        mskscene::HostTables a, b; std::string msg;
        CHECK(mskscene::pack(&s.d, nullptr, nullptr, &a, &msg) == MSK_OK, "%s", msg.c_str());
        CHECK(mskscene::pack(&s.d, nullptr, nullptr, &b, &msg, 0, nullptr) == MSK_OK, "%s", msg.c_str());
        CHECK(same(a.bsdfs, b.bsdfs) && same(a.texels, b.texels) && same(a.emitters, b.emitters) && same(a.tv, b.tv) && a.n_bsdf_f4 == b.n_bsdf_f4, "no masks: tables differ");
        CHECK(!b.has_mask && !b.has_mask_image && b.mask_base == 0 && a.all_diffuse == b.all_diffuse, "no masks: flags");
        CHECK(a.n_bsdf_f4 == 3u * MSK_BSDF_F4 + (bm ? 3u : 0u), "n_bsdf_f4 %u", a.n_bsdf_f4);
        // ---- layout: a constant on entry 1, a 3 x 2 bilinear image on entry 0, a 2 x 2 nearest one on entry 2
        const float img[6] = {0.f, 0.25f, 0.5f, 0.75f, 1.f, 0.125f}, img2[4] = {1.f, 0.f, 0.f, 1.f};
        const msk_mask_desc masks[3] = {constant_mask(1, 0.375f), image_mask(0, 2, 3, 2, img), image_mask(2, 1, 2, 2, img2)};
        mskscene::HostTables m;
        CHECK(mskscene::pack(&s.d, nullptr, nullptr, &m, &msg, 3, masks) == MSK_OK, "%s", msg.c_str());
        CHECK(m.has_mask && m.has_mask_image && !m.all_diffuse, "flags");
        CHECK(m.mask_base == a.n_bsdf_f4 && m.n_bsdf_f4 == a.n_bsdf_f4 + 9u, "mask_base %u n_bsdf_f4 %u", m.mask_base, m.n_bsdf_f4);
        CHECK(m.bsdfs.size() == (size_t) m.n_bsdf_f4 * 4, "bsdfs size");
        CHECK(!std::memcmp(m.bsdfs.data(), a.bsdfs.data(), a.bsdfs.size() * 4), "the records in front of the mask records changed");
        // the pool: the bitmap's texels (float4 each), then the values, floats, padded to a float4
        const size_t pool0 = bm ? 2u * 4u : 0u;
        CHECK(m.texels.size() == pool0 + 12u, "texels %zu", m.texels.size());
        if (bm) CHECK(!std::memcmp(m.texels.data(), a.texels.data(), pool0 * 4), "the bitmap's texels changed");
        const float *r0 = &m.bsdfs[(size_t) m.mask_base * 4], *r1 = r0 + 12, *r2 = r0 + 24;
        const size_t b0 = (size_t) m.mask_base * 4;
        CHECK(word(m.bsdfs, b0 + 12 + 4) == 0u && r1[5] == 0.375f, "constant record");
        CHECK(word(m.bsdfs, b0 + 4) == 2u && word(m.bsdfs, b0) == pool0 && word(m.bsdfs, b0 + 1) == 3u && word(m.bsdfs, b0 + 2) == 2u, "image record 0");
        CHECK(r0[3] == 0.125f && r0[7] == 0.75f && r0[8] == 4.f && r0[9] == 0.5f && r0[10] == -0.25f && r0[11] == 3.f, "to_uv of record 0");
        CHECK(word(m.bsdfs, b0 + 24 + 4) == 1u && word(m.bsdfs, b0 + 24) == pool0 + 6u && word(m.bsdfs, b0 + 25) == 2u && word(m.bsdfs, b0 + 26) == 2u, "image record 2");
        (void) r2;
        CHECK(!std::memcmp(&m.texels[pool0], img, 24) && !std::memcmp(&m.texels[pool0 + 6], img2, 16), "values");
        CHECK(m.texels[pool0 + 10] == 0.f && m.texels[pool0 + 11] == 0.f, "padding");
        // ---- one mask: the other entries carry the constant 1
        mskscene::HostTables one;
        CHECK(mskscene::pack(&s.d, nullptr, nullptr, &one, &msg, 1, masks) == MSK_OK, "%s", msg.c_str());
        CHECK(one.has_mask && !one.has_mask_image && one.texels.size() == (bm ? a.texels.size() : 0u), "a constant mask needs no pool of its own");
        for (int b2 : {0, 2}) CHECK(word(one.bsdfs, ((size_t) one.mask_base + 3u * b2 + 1u) * 4) == 0u && one.bsdfs[((size_t) one.mask_base + 3u * b2 + 1u) * 4 + 1] == 1.f, "entry %d: not the constant 1", b2);
        // ---- msk_plan.h's byte sums follow n_bsdf_f4, by what is staged and nothing else
        mskplan::TableCounts ca, cm;
        ca.n_tris = cm.n_tris = s.d.n_faces; ca.n_meshes = cm.n_meshes = 2; ca.n_emitters = cm.n_emitters = 1;
        ca.cdf_len = (uint32_t) a.cdf_all.size(); cm.cdf_len = (uint32_t) m.cdf_all.size();
        ca.n_bsdf_f4 = a.n_bsdf_f4; cm.n_bsdf_f4 = m.n_bsdf_f4;
        CHECK(mskplan::small_bytes(cm) == mskplan::small_bytes(ca) + 9u * 16u && mskplan::table_bytes(cm) == mskplan::table_bytes(ca) + 9u * 16u, "byte sums");
    }
    // ---- every refusal, by name
    const float ok_img[2] = {0.5f, 1.f}, bad_img[2] = {0.5f, 1.5f}, nan_img[2] = {NAN, 0.f}, neg_img[2] = {0.f, -0.f - 1e-9f};
    { const msk_mask_desc m[1] = {constant_mask(3, 0.5f)}; if (refusal("range", 1, m, "bsdf 3 out of range")) return 1; }
    { const msk_mask_desc m[2] = {constant_mask(1, 0.5f), constant_mask(1, 0.25f)}; if (refusal("twice", 2, m, "already has a mask")) return 1; }
    { const msk_mask_desc m[1] = {constant_mask(0, 1.5f)}; if (refusal("above", 1, m, "not in [0, 1]")) return 1; }
    { const msk_mask_desc m[1] = {constant_mask(0, -0.25f)}; if (refusal("below", 1, m, "not in [0, 1]")) return 1; }
    { const msk_mask_desc m[1] = {constant_mask(0, NAN)}; if (refusal("nan", 1, m, "not in [0, 1]")) return 1; }
    { const msk_mask_desc m[1] = {constant_mask(0, INFINITY)}; if (refusal("inf", 1, m, "not in [0, 1]")) return 1; }
    { msk_mask_desc m[1] = {constant_mask(0, 0.5f)}; m[0].filter = 3; if (refusal("filter 3", 1, m, "filter 3")) return 1; }
    { msk_mask_desc m[1] = {constant_mask(0, 0.5f)}; m[0].filter = -1; if (refusal("filter -1", 1, m, "filter -1")) return 1; }
    { const msk_mask_desc m[1] = {image_mask(0, 2, 0, 2, ok_img)}; if (refusal("zero width", 1, m, "0 x 2")) return 1; }
    { const msk_mask_desc m[1] = {image_mask(0, 1, 2, 0, ok_img)}; if (refusal("zero height", 1, m, "2 x 0")) return 1; }
    { const msk_mask_desc m[1] = {image_mask(0, 1, 2, 1, nullptr)}; if (refusal("no values", 1, m, "values array is missing")) return 1; }
    { const msk_mask_desc m[1] = {image_mask(0, 2, 2, 1, bad_img)}; if (refusal("value above", 1, m, "value 1")) return 1; }
    { const msk_mask_desc m[1] = {image_mask(0, 2, 2, 1, nan_img)}; if (refusal("value nan", 1, m, "value 0")) return 1; }
    { const msk_mask_desc m[1] = {image_mask(0, 2, 2, 1, neg_img)}; if (refusal("value below", 1, m, "value 1")) return 1; }
    if (refusal("null masks", 2, nullptr, "without masks")) return 1;
    {   // the limits themselves are taken: 0, 1, -0
        Scene s; make(s, false);
        const float edge[3] = {0.f, 1.f, -0.f};
        const msk_mask_desc m[3] = {constant_mask(0, 0.f), constant_mask(1, 1.f), image_mask(2, 1, 3, 1, edge)};
        mskscene::HostTables t; std::string msg;
        CHECK(mskscene::pack(&s.d, nullptr, nullptr, &t, &msg, 3, m) == MSK_OK, "%s", msg.c_str());
    }
    std::printf("ok %d\n", n_checks);
    return 0;
}
