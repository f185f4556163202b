// plastic_tables_check.cpp — the `plastic` part of scene creation's host side on a CPU, for tests/test_plastic_bsdf.py: what
// csrc/msk_scene_tables.h (through msk_plastic_tables.h) packs for an MSK_BSDF_PLASTIC entry: every refusal; fdr_int against a float64
// quadrature of another shape (from the inside, the kink at the critical angle substituted away) to 2e-7 relative, one fp32
// rounding; ssw against a float64 restatement to 1e-6 for a constant, a checkerboard, a bitmap and the both-zero case; a scene
// without a plastic packing to the bytes it had before the type existed (a recorded digest of every table); mask records of
// opacity 1 added exactly when the scene holds no mask.  Stand-alone; built with and without -fsanitize=address,undefined.
// Prints "ok <checks>" and returns 0, or the first failure and 1.
//   plastic_tables_check plan   csrc/msk_plan.h over the cross product of mask_tables_check.cpp's plan mode: with
//                               SceneFacts::has_plastic the plan is, field for field, the plan of the same facts with has_mask (SHADE_MASK,
//                               or SHADE_LENS with a lens); without it nothing changes.  Prints "cases N".
#include "../../misaki-render_amd/csrc/msk_scene_tables.h"
#include "../../misaki-render_amd/csrc/msk_lens_tables.h"
#include "../../misaki-render_amd/csrc/msk_plan.h"

#include <cmath>
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
// a plastic with the hosts' defaults: rho = 0.5 and s = 1 as uniform spectra, 1.49 / 1.00028, linear, one-sided
static msk_bsdf_desc plastic(float eta = 1.49f / 1.00028f) {
    msk_bsdf_desc b = diffuse(0.f);
    b.type = MSK_BSDF_PLASTIC;
    b.reflectance[0] = 0.f; b.reflectance[1] = 0.f; b.reflectance[2] = INFINITY; b.reflectance_scale = 0.5f;
    b.ior_eta = eta; b.ior_inv_eta = 1.f / eta;
    b.alpha_u = -1.f; b.alpha_v = NAN;          // ignored: not the roughness check's business
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
// mask_tables_check.cpp's scene: two quads, three BSDF entries (the last unreferenced), one area emitter, a checkerboard (texture 1)
// and a 2 x 2 bitmap (texture 2) that entry 0 uses when with_bitmap
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
    msk_texture_desc c;
    std::memset(&c, 0, sizeof c);
    c.type = MSK_TEXTURE_CHECKERBOARD; c.to_uv[0] = 4.f; c.to_uv[4] = 4.f;
    c.color0[0] = 0.001f; c.color0[1] = -1.1f; c.color0[2] = 300.f; c.color1[0] = -0.0004f; c.color1[1] = 0.45f; c.color1[2] = -120.f;
    s.textures.push_back(c);
    msk_texture_desc t;
    std::memset(&t, 0, sizeof t);
    t.type = MSK_TEXTURE_BITMAP; t.width = 2; t.height = 2; t.first_texel = 1; t.to_uv[0] = 1.f; t.to_uv[4] = 1.f;
    s.textures.push_back(t);
    const float tx[5][3] = {{9.f, 9.f, 9.f}, {0.f, 0.f, INFINITY}, {0.f, 0.f, -INFINITY}, {0.0008f, -0.9f, 250.f}, {-0.0002f, 0.2f, -50.f}};      // texel 0 is not the bitmap's
    for (const auto &k : tx) s.texels.insert(s.texels.end(), k, k + 3);
    if (with_bitmap) s.bsdfs[0].reflectance_texture = 2;
    s.d.n_meshes = (uint32_t) s.meshes.size(); s.d.meshes = s.meshes.data();
    s.d.n_bsdfs = (uint32_t) s.bsdfs.size(); s.d.bsdfs = s.bsdfs.data();
    s.d.n_emitters = 1; s.d.emitters = s.emitters.data();
    s.d.n_vertices = (uint32_t) (s.vertices.size() / 8); s.d.vertices = s.vertices.data();
    s.d.n_faces = (uint32_t) (s.faces.size() / 3); s.d.faces = s.faces.data();
    s.d.n_textures = (uint32_t) s.textures.size(); s.d.textures = s.textures.data();
    s.d.n_texels = (uint32_t) (s.texels.size() / 3); s.d.texels = s.texels.data();
    s.d.cie1931_xyz = s.cie; s.d.d65 = s.d65;
}
static uint32_t word(const std::vector<float> &v, size_t i) { uint32_t w; std::memcpy(&w, &v[i], 4); return w; }

// FNV-1a over every table pack() returns
static uint64_t digest(const mskscene::HostTables &t) {
    uint64_t h = 1469598103934665603ull;
    auto eat = [&](const void *p, size_t n) { const unsigned char *c = (const unsigned char *) p; for (size_t i = 0; i < n; ++i) { h ^= c[i]; h *= 1099511628211ull; } };
    for (const std::vector<float> *v : {&t.pos, &t.tv, &t.tn, &t.tuv, &t.bsdfs, &t.emitters, &t.d65, &t.emitter_grid, &t.cdf_all, &t.spectra_pool, &t.cie, &t.texels})
        { const size_t n = v->size(); eat(&n, sizeof n); if (n) eat(v->data(), n * 4); }
    eat(t.mesh_info.data(), t.mesh_info.size() * 4); eat(t.bsdf_types.data(), t.bsdf_types.size() * 4);
    const uint32_t w[4] = {t.n_bsdf_f4, t.tex_base, t.mask_base, (uint32_t) t.all_diffuse | (uint32_t) t.has_bitmap << 1 | (uint32_t) t.has_mask << 2};
    eat(w, sizeof w); eat(&t.tri_pad, 4);
    return h;
}

// ---- float64 restatements
// the exact unpolarised reflectance of a boundary from index n1 into n2 at cos(theta_i) = ci: Snell, then the two amplitude ratios
static double fresnel_textbook(double ci, double n1, double n2) {
    const double si2 = (n1 / n2) * (n1 / n2) * (1.0 - ci * ci);
    if (si2 >= 1.0) return 1.0;
    const double ct = std::sqrt(1.0 - si2);
    const double rs = (n1 * ci - n2 * ct) / (n1 * ci + n2 * ct), rp = (n1 * ct - n2 * ci) / (n1 * ct + n2 * ci);
    return 0.5 * (rs * rs + rp * rp);
}
// 2 int_0^1 F(mu; from inside) mu dmu: total reflection below mu_c = sqrt(1 - 1 / eta^2) gives mu_c^2; above it, with t = the cosine
// outside in [0, 1] (mu^2 = mu_c^2 + t^2 / eta^2, 2 mu dmu = 2 t dt / eta^2), composite Simpson on 2^14 panels of a smooth integrand
static double fdr_int_direct(double eta) {
    if (eta == 1.0) return 0.0;
    const double mu_c2 = 1.0 - 1.0 / (eta * eta);
    const int n = 1 << 14;
    auto f = [&](double t) { const double mu = std::sqrt(mu_c2 + t * t / (eta * eta)); return fresnel_textbook(mu, eta, 1.0) * 2.0 * t / (eta * eta); };
    double s = f(0.0) + f(1.0);
    for (int i = 1; i < n; ++i) s += f((double) i / n) * ((i & 1) ? 4.0 : 2.0);
    return mu_c2 + s / (3.0 * n);
}
static double sigmoid(const float *c, double l) {
    if (std::isinf(c[2])) return c[2] > 0 ? 1.0 : 0.0;
    const double x = ((double) c[0] * l + c[1]) * l + c[2];
    return std::fmax(0.5 + x / (2.0 * std::sqrt(1.0 + x * x)), 0.0);
}
static double mean95(const float *c) { long double s = 0; for (int i = 0; i < 95; ++i) s += sigmoid(c, 360.0 + 5.0 * i); return (double) (s / 95); }

static int pack_one(Scene &s, mskscene::HostTables *t, uint32_t n_masks = 0, const msk_mask_desc *masks = nullptr) {
    std::string msg;
    const int rc = mskscene::pack(&s.d, nullptr, nullptr, t, &msg, n_masks, masks);
    if (rc) std::printf("pack: %s\n", msg.c_str());
    return rc;
}
static int refusal(const char *name, const msk_bsdf_desc &bd, const char *words, int code = MSK_ERR_INVALID_ARG) {
    Scene s; make(s, false);
    s.bsdfs[1] = bd;
    mskscene::HostTables t; std::string msg;
    const int rc = mskscene::pack(&s.d, nullptr, nullptr, &t, &msg);
    CHECK(rc == code, "%s: code %d, message \"%s\"", name, rc, msg.c_str());
    CHECK(msg.find(words) != std::string::npos, "%s: \"%s\" does not say \"%s\"", name, msg.c_str(), words);
    CHECK(msg.find("bsdf 1") != std::string::npos, "%s: \"%s\" does not name the entry", name, msg.c_str());
    return 0;
}

#define FIELDS(X) X(shade_kind) X(lds_tables) X(diffuse_only) X(regular) X(dielectric) X(sort_on) X(shade_lds_bytes) X(trace_family) X(trace_mode) X(refill) \
    X(max_inner) X(queue_refill) X(trace_lds_bytes) X(bits_off) X(trace_waves) X(trace_split) X(lane_refill) X(fused_ok) X(fused_h) X(fused_all) \
    X(fused_iters) X(fused_tail_pct) X(fused_lds_bytes) X(fused_queue_f4) X(fused_trace_f4) X(cull) X(sync_group) X(timing_every)
static int plan_check() {
    using namespace mskplan;
    const RenderKnobs knobs = read_render_knobs();
    static const size_t lds[7][2] = {{24576, 8192}, {53248, 8192}, {53264, 8192}, {24576, 65024}, {24576, 65040}, {24576, 40960}, {24576, 40976}};
    static const uint32_t region_sizes[4] = {256, 1024, 2048, 8192};
    if (SceneFacts().has_plastic) { std::printf("has_plastic must default to false\n"); return 1; }
    unsigned long n = 0;
    for (int mode = 0; mode <= 6; ++mode)
        for (int flags = 0; flags < 1024; ++flags)
            for (int aov = 0; aov < 4; ++aov)
                for (uint32_t rs : region_sizes)
                    for (const auto &l : lds) {
                        SceneFacts s;
                        s.trace_mode = mode; s.lds_scene = mode == TRACE_BIN_LDS || mode == TRACE_WIDE4_LDS;
                        s.lds_tables = flags & 1; s.all_diffuse = false; s.has_regular = flags & 4; s.has_dielectric = flags & 8; s.cull_ok = flags & 16;
                        s.has_bitmap = flags & 32; s.has_envmap = flags & 64; s.has_delta = flags & 128; s.has_mask = flags & 256; s.has_lens = flags & 512;
                        if (flags & 2) continue;                          // (all_diffuse is never set beside a plastic: the packer clears it)
                        s.shade_lds_bytes = l[0]; s.trace_lds_bytes = l[1];
                        CallFacts c;
                        c.region_size = rs; c.aov_groups = (aov & 1) ? 2u : 0u; c.aov_rgb = (aov & 2) != 0;
                        SceneFacts sp = s, sm = s;
                        sp.has_plastic = true; sm.has_mask = true;
                        const LaunchPlan e = make_launch_plan(sp, c, knobs), m = make_launch_plan(sm, c, knobs);
                        const char *bad = nullptr;
                        if (e.shade_kind != (s.has_lens ? SHADE_LENS : SHADE_MASK)) bad = "shade_kind (SHADE_MASK, or SHADE_LENS with a lens)";
                        if (shade_family(sp) != e.shade_kind) bad = "shade_family";
#define X(f) if (!(e.f == m.f)) bad = #f;
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
    static_assert(sizeof(msk_bsdf_desc) == 132, "msk_bsdf_desc keeps its size");
    static_assert(MSK_BSDF_PLASTIC == 6, "type 5 stays unassigned");
    // ---- a scene without a plastic packs to the bytes it had before the type existed: digests recorded from the parent's packer
    for (int bm = 0; bm < 2; ++bm) {
        Scene s; make(s, bm);
        mskscene::HostTables a;
        CHECK(pack_one(s, &a) == MSK_OK, "pack");
        CHECK(!a.has_plastic && !a.has_mask && a.mask_base == 0 && a.n_bsdf_f4 == 3u * MSK_BSDF_F4 + 6u, "no plastic: n_bsdf_f4 %u", a.n_bsdf_f4);
        static const uint64_t recorded[2] = {0xee0d6d5261372e30ull, 0x15186cf1e90b2cc9ull};
        CHECK(digest(a) == recorded[bm], "the tables of a scene without a plastic changed: 0x%016llx", (unsigned long long) digest(a));
    }
    // ---- type 5 keeps its refusal, word for word
    {
        msk_bsdf_desc b = plastic(); b.type = 5;
        if (refusal("type 5", b, "bsdf 1: type 5 is not supported by this back end (diffuse, roughconductor, roughdielectric, dielectric, conductor)", MSK_ERR_UNSUPPORTED)) return 1;
    }
    // ---- every refusal of a type-6 descriptor
    { msk_bsdf_desc b = plastic(); b.ior_eta = 0.999f; if (refusal("eta below 1", b, "ior_eta")) return 1; }
    { msk_bsdf_desc b = plastic(); b.ior_eta = NAN; if (refusal("eta nan", b, "ior_eta")) return 1; }
    { msk_bsdf_desc b = plastic(); b.ior_eta = INFINITY; if (refusal("eta inf", b, "ior_eta")) return 1; }
    { msk_bsdf_desc b = plastic(); b.ior_eta = -1.5f; if (refusal("eta negative", b, "ior_eta")) return 1; }
    { msk_bsdf_desc b = plastic(); b.ior_inv_eta = 0.f; if (refusal("inv_eta zero", b, "ior_inv_eta")) return 1; }
    { msk_bsdf_desc b = plastic(); b.ior_inv_eta = NAN; if (refusal("inv_eta nan", b, "ior_inv_eta")) return 1; }
    { msk_bsdf_desc b = plastic(); b.back_bsdf = 3; if (refusal("back_bsdf", b, "back_bsdf 3 out of range")) return 1; }
    { msk_bsdf_desc b = plastic(); b.reflectance_scale = -0.5f; if (refusal("negative rho", b, "reflectance_scale")) return 1; }
    { msk_bsdf_desc b = plastic(); b.reflectance_scale = INFINITY; if (refusal("infinite rho", b, "reflectance_scale")) return 1; }
    { msk_bsdf_desc b = plastic(); b.reflectance_texture = 3; if (refusal("texture range", b, "reflectance_texture 3 out of range")) return 1; }
    { msk_bsdf_desc b = plastic(); b.reflectance_regular = 1; if (refusal("regular range", b, "regular spectrum 1 of 0")) return 1; }
    { msk_bsdf_desc b = plastic(); b.specular_reflectance.scale = -1.f; if (refusal("negative s", b, "specular_reflectance")) return 1; }
    { msk_bsdf_desc b = plastic(); b.specular_reflectance.scale = INFINITY; if (refusal("infinite s", b, "specular_reflectance")) return 1; }
    { msk_bsdf_desc b = plastic(); b.specular_reflectance.regular = 2; if (refusal("s regular range", b, "specular_reflectance names regular spectrum 2 of 0")) return 1; }
    // ---- the record, the constants, the mask records
    const float etas[4] = {1.f, 1.2f, 1.4896f, 1.9f};
    for (float eta : etas)
        for (int kind = 0; kind < 5; ++kind) {      // rho: 0 constant, 1 checkerboard, 2 bitmap, 3 black with s = 0 (both zero), 4 black with s = 0.7 (ssw = 1)
            Scene s; make(s, false);
            msk_bsdf_desc b = plastic(eta);
            b.back_bsdf = 1; b.sample_visible = kind == 1 ? 7 : 0;
            const float sc[3] = {0.0006f, -0.7f, 200.f};
            std::memcpy(b.specular_reflectance.coeff, sc, 12); b.specular_reflectance.scale = 0.7f;
            double d_mean = 0.0, s_mean = 0.7 * mean95(sc);
            if (kind == 0) { const float rc[3] = {-0.0003f, 0.3f, -70.f}; std::memcpy(b.reflectance, rc, 12); b.reflectance_scale = 0.8f; d_mean = 0.8 * mean95(rc); }
            if (kind == 1) { b.reflectance_texture = 1; d_mean = 0.5 * (mean95(s.textures[0].color0) + mean95(s.textures[0].color1)); }
            if (kind == 2) { b.reflectance_texture = 2; for (int k = 1; k < 5; ++k) d_mean += 0.25 * mean95(&s.texels[k * 3]); }
            if (kind >= 3) b.reflectance_scale = 0.f;
            if (kind == 3) { b.specular_reflectance.scale = 0.f; s_mean = 0.0; }
            s.bsdfs[1] = b;
            mskscene::HostTables t;
            CHECK(pack_one(s, &t) == MSK_OK, "pack");
            CHECK(t.has_plastic && !t.has_mask && !t.all_diffuse && t.bsdf_types[1] == MSK_BSDF_PLASTIC, "flags");
            const float *o = &t.bsdfs[(size_t) 1 * 4 * MSK_BSDF_F4];
            const double want_fdr = fdr_int_direct((double) eta), want_ssw = d_mean + s_mean > 0 ? s_mean / (d_mean + s_mean) : 1.0;
            CHECK(std::fabs((double) o[5] - want_fdr) <= 2e-7 * want_fdr, "fdr_int(%g) = %.9g, float64 %.12g", (double) eta, (double) o[5], want_fdr);
            CHECK(std::fabs((double) o[6] - want_ssw) <= 1e-6, "ssw kind %d = %.9g, float64 %.12g", kind, (double) o[6], want_ssw);
            if (eta == 1.f) CHECK(o[5] == 0.f, "fdr_int(1) is exactly 0");
            if (kind >= 3) CHECK(o[6] == 1.f, "ssw of a black base (or of nothing at all) is exactly 1");
            CHECK(word(t.bsdfs, (size_t) 1 * 4 * MSK_BSDF_F4 + 7) == (kind == 1 ? 1u : 0u), "nonlinear is 0 or 1");
            CHECK(word(t.bsdfs, (size_t) 1 * 4 * MSK_BSDF_F4) == 6u && word(t.bsdfs, (size_t) 1 * 4 * MSK_BSDF_F4 + 1) == 1u, "type, back_bsdf");
            CHECK(o[24] == eta && o[25] == 1.f / eta && o[19] == b.specular_reflectance.scale, "ior, s");
            CHECK(o[27] == b.reflectance_scale && word(t.bsdfs, (size_t) 1 * 4 * MSK_BSDF_F4 + 26) == (b.reflectance_texture ? 3u * MSK_BSDF_F4 + (b.reflectance_texture - 1u) * 3u : 0u), "rho");
            // the other entries' records, and the texture records, are those of the scene with a diffuse entry 1
            Scene s0; make(s0, false);
            mskscene::HostTables t0;
            CHECK(pack_one(s0, &t0) == MSK_OK, "pack");
            CHECK(t.mask_base == t0.n_bsdf_f4 && t.n_bsdf_f4 == t0.n_bsdf_f4 + 9u && t.bsdfs.size() == (size_t) t.n_bsdf_f4 * 4, "mask records: base %u", t.mask_base);
            CHECK(!std::memcmp(t.bsdfs.data(), t0.bsdfs.data(), 4 * MSK_BSDF_F4 * 4) && !std::memcmp(&t.bsdfs[8 * MSK_BSDF_F4], &t0.bsdfs[8 * MSK_BSDF_F4], (t0.bsdfs.size() - 8 * MSK_BSDF_F4) * 4), "records around the plastic changed");
            for (uint32_t e = 0; e < 3; ++e) {
                const size_t r = ((size_t) t.mask_base + 3u * e) * 4;
                for (int k = 0; k < 12; ++k) CHECK(word(t.bsdfs, r + k) == (k == 5 ? 0x3f800000u : 0u), "entry %u word %d: not {filter 0, opacity 1}", e, k);
            }
            // with a mask of its own: the mask's records and no others; with a lens on top: still one set
            msk_mask_desc m;
            std::memset(&m, 0, sizeof m);
            m.bsdf = 1; m.opacity = 0.25f;
            mskscene::HostTables tm;
            CHECK(pack_one(s, &tm, 1, &m) == MSK_OK, "pack");
            CHECK(tm.has_mask && tm.has_plastic && tm.n_bsdf_f4 == t.n_bsdf_f4 && tm.mask_base == t.mask_base && tm.bsdfs[((size_t) tm.mask_base + 4u) * 4 + 1] == 0.25f, "mask over plastic");
            CHECK(!std::memcmp(tm.bsdfs.data(), t.bsdfs.data(), (size_t) t.mask_base * 16), "a mask changed the plastic's record");
            mskscene::HostTables tl = t;
            mskscene::add_lens_tables(&s.d, &tl);
            CHECK(tl.n_bsdf_f4 == t.n_bsdf_f4 && tl.bsdfs.size() == t.bsdfs.size() && !std::memcmp(tl.bsdfs.data(), t.bsdfs.data(), t.bsdfs.size() * 4) && !tl.all_diffuse, "a lens added a second set of mask records");
        }
    // fdr_int falls with nothing but eta: the same for every entry that shares it; and it grows with eta
    {
        Scene s; make(s, false);
        s.bsdfs[0] = plastic(1.3f); s.bsdfs[1] = plastic(1.3f); s.bsdfs[2] = plastic(1.7f);
        s.bsdfs[1].reflectance_scale = 0.9f;
        mskscene::HostTables t;
        CHECK(pack_one(s, &t) == MSK_OK, "pack");
        CHECK(t.bsdfs[5] == t.bsdfs[4 * MSK_BSDF_F4 + 5] && t.bsdfs[8 * MSK_BSDF_F4 + 5] > t.bsdfs[5] && t.bsdfs[5] > 0.3f && t.bsdfs[8 * MSK_BSDF_F4 + 5] < 0.8f, "fdr_int over eta");
        CHECK(t.bsdfs[6] > t.bsdfs[4 * MSK_BSDF_F4 + 6], "ssw falls as rho grows");
    }
    std::printf("ok %d\n", n_checks);
    return 0;
}
