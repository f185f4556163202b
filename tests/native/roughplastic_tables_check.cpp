// roughplastic_tables_check.cpp — the `roughplastic` part of scene creation's host side on a CPU, for tests/test_roughplastic_bsdf.py:
// what csrc/msk_scene_tables.h (through msk_plastic_tables.h) packs for an MSK_BSDF_ROUGHPLASTIC entry: every refusal text (type 6's
// checks under the type's own name, a negative or non-finite alpha, alpha_u != alpha_v by the word "anisotropic"), type 5's
// unchanged words, the record layout of type 7 (alpha in word 5, nonlinear in word 7, {fdr_int, ssw} in words 20 and 21), type 6's
// record and a scene without a plastic packing to recorded digests, and the constants against float64 with the plastic's bounds (2e-7
// relative, 1e-6).  Stand-alone; built with and without -fsanitize=address,undefined.  Prints "ok <checks>" and returns 0, or the
// first failure and 1.
//   roughplastic_tables_check plan      a type-7 scene's facts plan SHADE_MASK, or SHADE_LENS with a lens, whatever else they hold
//   roughplastic_tables_check digests   prints the three digests the default mode holds recorded
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
// the hosts' defaults: rho = 0.5 and s = 1 as uniform spectra, 1.49 / 1.00028, linear, one-sided; type 6, or type 7 with alpha 0.1
static msk_bsdf_desc plastic(int type, float eta = 1.49f / 1.00028f, float alpha = 0.1f) {
    msk_bsdf_desc b = diffuse(0.f);
    b.type = type;
    b.reflectance[0] = 0.f; b.reflectance[1] = 0.f; b.reflectance[2] = INFINITY; b.reflectance_scale = 0.5f;
    b.ior_eta = eta; b.ior_inv_eta = 1.f / eta;
    b.alpha_u = b.alpha_v = alpha;
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
// plastic_tables_check.cpp's scene: two quads, three BSDF entries (the last unreferenced), one area emitter, a checkerboard (texture 1)
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
    const uint32_t w[4] = {t.n_bsdf_f4, t.tex_base, t.mask_base, (uint32_t) t.all_diffuse | (uint32_t) t.has_bitmap << 1 | (uint32_t) t.has_mask << 2 | (uint32_t) t.has_plastic << 3};
    eat(w, sizeof w); eat(&t.tri_pad, 4);
    return h;
}

// ---- float64 restatements (plastic_tables_check.cpp's)
static double fresnel_textbook(double ci, double n1, double n2) {
    const double si2 = (n1 / n2) * (n1 / n2) * (1.0 - ci * ci);
    if (si2 >= 1.0) return 1.0;
    const double ct = std::sqrt(1.0 - si2);
    const double rs = (n1 * ci - n2 * ct) / (n1 * ci + n2 * ct), rp = (n1 * ct - n2 * ci) / (n1 * ct + n2 * ci);
    return 0.5 * (rs * rs + rp * rp);
}
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
// the scene with a type-6 entry 1 whose digest is recorded: coloured rho and s, twosided, nonlinear
static void type6_scene(Scene &s) {
    make(s, true);
    msk_bsdf_desc b = plastic(6, 1.4896f, 0.f);
    const float sc[3] = {0.0006f, -0.7f, 200.f}, rc[3] = {-0.0003f, 0.3f, -70.f};
    std::memcpy(b.specular_reflectance.coeff, sc, 12); b.specular_reflectance.scale = 0.7f;
    std::memcpy(b.reflectance, rc, 12); b.reflectance_scale = 0.8f;
    b.back_bsdf = 1; b.sample_visible = 7;
    s.bsdfs[1] = b;
}
static const uint64_t kRecorded[3] = {0xee0d6d5261372e30ull, 0x15186cf1e90b2cc9ull, 0xeee051c97fa2d3c7ull};       // no plastic, no plastic with a bitmap, type6_scene
static int digests(uint64_t out[3]) {
    for (int bm = 0; bm < 2; ++bm) { Scene s; make(s, bm); mskscene::HostTables a; if (pack_one(s, &a)) return 1; out[bm] = digest(a); }
    Scene s; type6_scene(s); mskscene::HostTables a; if (pack_one(s, &a)) return 1; out[2] = digest(a);
    return 0;
}

static int plan_check() {
    using namespace mskplan;
    const RenderKnobs knobs = read_render_knobs();
    unsigned long n = 0;
    for (int lens = 0; lens < 2; ++lens)
        for (int with_mask = 0; with_mask < 2; ++with_mask)
            for (int mode = 0; mode <= 6; ++mode)
                for (int flags = 0; flags < 64; ++flags) {
                    Scene s; make(s, flags & 1);
                    s.bsdfs[1] = plastic(MSK_BSDF_ROUGHPLASTIC);
                    msk_mask_desc m;
                    std::memset(&m, 0, sizeof m);
                    m.bsdf = 1; m.opacity = 0.5f;
                    mskscene::HostTables t;
                    if (pack_one(s, &t, with_mask, &m)) return 1;
                    if (lens) mskscene::add_lens_tables(&s.d, &t);
                    SceneFacts f;                                // as msk_gpu_scene_create_lens fills them
                    f.trace_mode = mode; f.lds_scene = mode == TRACE_BIN_LDS || mode == TRACE_WIDE4_LDS;
                    f.lds_tables = flags & 2; f.shade_lds_bytes = 24576; f.trace_lds_bytes = 8192; f.cull_ok = flags & 4;
                    f.all_diffuse = t.all_diffuse; f.has_regular = t.has_regular || (flags & 8); f.has_dielectric = t.has_dielectric || (flags & 16); f.has_bitmap = t.has_bitmap;
                    f.has_envmap = t.has_envmap; f.has_delta = t.has_delta || (flags & 32); f.has_mask = t.has_mask; f.has_plastic = t.has_plastic; f.has_lens = lens;
                    if (!t.has_plastic || t.all_diffuse || t.has_mask != (bool) with_mask) { std::printf("facts of a type-7 scene\n"); return 1; }
                    CallFacts c;
                    c.region_size = 1024;
                    const ShadeKind want = lens ? SHADE_LENS : SHADE_MASK;
                    if (shade_family(f) != want || make_launch_plan(f, c, knobs).shade_kind != want) {
                        std::printf("a type-7 scene plans kind %d, not %d: lens %d mask %d mode %d flags %d\n", (int) make_launch_plan(f, c, knobs).shade_kind, (int) want, lens, with_mask, mode, flags);
                        return 1;
                    }
                    ++n;
                }
    std::printf("cases %lu\n", n);
    return 0;
}

int main(int argc, char **argv) {
    if (argc > 1 && std::string(argv[1]) == "plan") return plan_check();
    uint64_t got[3];
    if (digests(got)) return 1;
    if (argc > 1 && std::string(argv[1]) == "digests") { std::printf("0x%016llxull, 0x%016llxull, 0x%016llxull\n", (unsigned long long) got[0], (unsigned long long) got[1], (unsigned long long) got[2]); return 0; }
    static_assert(sizeof(msk_bsdf_desc) == 132, "msk_bsdf_desc keeps its size");
    static_assert(MSK_BSDF_PLASTIC == 6 && MSK_BSDF_ROUGHPLASTIC == 7, "type 5 stays unassigned");
    // ---- a scene without a plastic, and one with a type 6, pack to the bytes the packer gave before type 7 existed
    for (int k = 0; k < 3; ++k) CHECK(got[k] == kRecorded[k], "tables %d changed: 0x%016llx", k, (unsigned long long) got[k]);
    {
        Scene s; type6_scene(s);
        mskscene::HostTables t;
        CHECK(pack_one(s, &t) == MSK_OK, "pack");
        const size_t r = (size_t) 4 * MSK_BSDF_F4;
        CHECK(word(t.bsdfs, r) == 6u && word(t.bsdfs, r + 7) == 1u && t.bsdfs[r + 5] > 0.5f && t.bsdfs[r + 5] < 0.7f && t.bsdfs[r + 6] > 0.f && t.bsdfs[r + 6] < 1.f, "type 6: constants in words 5 and 6");
        CHECK(t.bsdfs[r + 20] == 0.f && t.bsdfs[r + 21] == 0.f && std::isinf(t.bsdfs[r + 22]) && t.bsdfs[r + 23] == 1.f, "type 6: specular_transmittance is the spectrum's record");
    }
    // ---- type 5 keeps its refusal, word for word
    {
        msk_bsdf_desc b = plastic(7); b.type = 5;
        if (refusal("type 5", b, "bsdf 1: type 5 is not supported by this back end (diffuse, roughconductor, roughdielectric, dielectric, conductor)", MSK_ERR_UNSUPPORTED)) return 1;
        b.type = 8;
        if (refusal("type 8", b, "bsdf 1: type 8 is not supported by this back end (diffuse, roughconductor, roughdielectric, dielectric, conductor)", MSK_ERR_UNSUPPORTED)) return 1;
    }
    // ---- every refusal of a type-7 descriptor: type 6's, under the type's name ...
    { msk_bsdf_desc b = plastic(7); b.ior_eta = 0.999f; if (refusal("eta below 1", b, "bsdf 1: roughplastic: the relative index of refraction ior_eta 0.999 must be finite and at least 1")) return 1; }
    { msk_bsdf_desc b = plastic(7); b.ior_eta = NAN; if (refusal("eta nan", b, "roughplastic: the relative index of refraction ior_eta")) return 1; }
    { msk_bsdf_desc b = plastic(7); b.ior_eta = INFINITY; if (refusal("eta inf", b, "roughplastic: the relative index of refraction ior_eta")) return 1; }
    { msk_bsdf_desc b = plastic(7); b.ior_eta = -1.5f; if (refusal("eta negative", b, "roughplastic: the relative index of refraction ior_eta")) return 1; }
    { msk_bsdf_desc b = plastic(7); b.ior_inv_eta = 0.f; if (refusal("inv_eta zero", b, "bsdf 1: roughplastic: ior_inv_eta 0 must be finite and positive")) return 1; }
    { msk_bsdf_desc b = plastic(7); b.ior_inv_eta = NAN; if (refusal("inv_eta nan", b, "roughplastic: ior_inv_eta")) return 1; }
    { msk_bsdf_desc b = plastic(7); b.specular_reflectance.scale = INFINITY; if (refusal("infinite s", b, "specular_reflectance")) return 1; }
    { msk_bsdf_desc b = plastic(7); b.specular_reflectance.scale = -1.f; if (refusal("negative s", b, "specular_reflectance")) return 1; }
    { msk_bsdf_desc b = plastic(7); b.specular_reflectance.regular = 2; if (refusal("s regular range", b, "specular_reflectance names regular spectrum 2 of 0")) return 1; }
    { msk_bsdf_desc b = plastic(7); b.back_bsdf = 3; if (refusal("back_bsdf", b, "back_bsdf 3 out of range")) return 1; }
    { msk_bsdf_desc b = plastic(7); b.reflectance_scale = -0.5f; if (refusal("negative rho", b, "reflectance_scale")) return 1; }
    { msk_bsdf_desc b = plastic(7); b.reflectance_scale = INFINITY; if (refusal("infinite rho", b, "reflectance_scale")) return 1; }
    { msk_bsdf_desc b = plastic(7); b.reflectance_texture = 3; if (refusal("texture range", b, "reflectance_texture 3 out of range")) return 1; }
    { msk_bsdf_desc b = plastic(7); b.reflectance_regular = 1; if (refusal("regular range", b, "regular spectrum 1 of 0")) return 1; }
    // ... and the roughness's own
    { msk_bsdf_desc b = plastic(7); b.alpha_u = b.alpha_v = -0.1f; if (refusal("negative alpha", b, "bsdf 1: roughplastic: the roughness alpha (-0.1, -0.1) must be finite and non-negative")) return 1; }
    { msk_bsdf_desc b = plastic(7); b.alpha_u = b.alpha_v = NAN; if (refusal("nan alpha", b, "must be finite and non-negative")) return 1; }
    { msk_bsdf_desc b = plastic(7); b.alpha_u = b.alpha_v = INFINITY; if (refusal("infinite alpha", b, "must be finite and non-negative")) return 1; }
    { msk_bsdf_desc b = plastic(7); b.alpha_v = INFINITY; if (refusal("one infinite alpha", b, "must be finite and non-negative")) return 1; }
    { msk_bsdf_desc b = plastic(7); b.alpha_v = 0.2f; if (refusal("alpha_u != alpha_v", b, "bsdf 1: roughplastic: alpha_u 0.1 and alpha_v 0.2 differ: anisotropic coats are not supported")) return 1; }
    { msk_bsdf_desc b = plastic(7); b.alpha_u = 0.f; if (refusal("alpha_u != alpha_v (0)", b, "anisotropic")) return 1; }
    // ---- the record, the constants, the mask records
    const float etas[4] = {1.f, 1.2f, 1.4896f, 1.9f};
    const float alphas[4] = {0.f, 1e-5f, 0.3f, 1.f};
    for (int ei = 0; ei < 4; ++ei)
        for (int kind = 0; kind < 5; ++kind) {      // rho: 0 constant, 1 checkerboard, 2 bitmap, 3 black with s = 0 (both zero), 4 black with s = 0.7 (ssw = 1)
            const float eta = etas[ei], alpha = alphas[(ei + kind) % 4];
            Scene s; make(s, false);
            msk_bsdf_desc b = plastic(7, eta, alpha);
            b.back_bsdf = 1; b.sample_visible = kind == 1 ? 7 : 0;
            const float sc[3] = {0.0006f, -0.7f, 200.f};
            std::memcpy(b.specular_reflectance.coeff, sc, 12); b.specular_reflectance.scale = 0.7f;
            b.specular_transmittance.scale = 0.25f;        // ignored, and its first two words overwritten
            double d_mean = 0.0, s_mean = 0.7 * mean95(sc);
            if (kind == 0) { const float rc[3] = {-0.0003f, 0.3f, -70.f}; std::memcpy(b.reflectance, rc, 12); b.reflectance_scale = 0.8f; d_mean = 0.8 * mean95(rc); }
            if (kind == 1) { b.reflectance_texture = 1; d_mean = 0.5 * (mean95(s.textures[0].color0) + mean95(s.textures[0].color1)); }
            if (kind == 2) { b.reflectance_texture = 2; for (int k = 1; k < 5; ++k) d_mean += 0.25 * mean95(&s.texels[k * 3]); }
            if (kind >= 3) b.reflectance_scale = 0.f;
            if (kind == 3) { b.specular_reflectance.scale = 0.f; s_mean = 0.0; }
            s.bsdfs[1] = b;
            mskscene::HostTables t;
            CHECK(pack_one(s, &t) == MSK_OK, "pack");
            CHECK(t.has_plastic && !t.has_mask && !t.all_diffuse && t.bsdf_types[1] == MSK_BSDF_ROUGHPLASTIC, "flags");
            const size_t r = (size_t) 1 * 4 * MSK_BSDF_F4;
            const float *o = &t.bsdfs[r];
            const double want_fdr = fdr_int_direct((double) eta), want_ssw = d_mean + s_mean > 0 ? s_mean / (d_mean + s_mean) : 1.0;
            CHECK(mskscene::plastic_constants_word(7) == 20u && mskscene::plastic_constants_word(6) == 5u, "where the constants stand");
            CHECK(std::fabs((double) o[20] - want_fdr) <= 2e-7 * want_fdr, "fdr_int(%g) = %.9g, float64 %.12g", (double) eta, (double) o[20], want_fdr);
            CHECK(std::fabs((double) o[21] - want_ssw) <= 1e-6, "ssw kind %d = %.9g, float64 %.12g", kind, (double) o[21], want_ssw);
            if (eta == 1.f) CHECK(o[20] == 0.f, "fdr_int(1) is exactly 0");
            if (kind >= 3) CHECK(o[21] == 1.f, "ssw of a black base (or of nothing at all) is exactly 1");
            CHECK(o[5] == alpha && o[6] == alpha, "alpha stays where the rough types keep alpha_u (unclamped: the clamp is applied at use)");
            CHECK(word(t.bsdfs, r + 7) == (kind == 1 ? 1u : 0u), "nonlinear is 0 or 1");
            CHECK(word(t.bsdfs, r) == 7u && word(t.bsdfs, r + 1) == 1u, "type, back_bsdf");
            CHECK(std::isinf(o[22]) && o[23] == 0.25f, "the last two words of `trans` are the spectrum record's");
            CHECK(o[24] == eta && o[25] == 1.f / eta && o[19] == b.specular_reflectance.scale, "ior, s");
            CHECK(o[27] == b.reflectance_scale && word(t.bsdfs, r + 26) == (b.reflectance_texture ? 3u * MSK_BSDF_F4 + (b.reflectance_texture - 1u) * 3u : 0u), "rho");
            // the same descriptor as a type 6 gives the same constants, in its own words, and the same words elsewhere
            Scene s6; make(s6, false);
            s6.bsdfs[1] = b; s6.bsdfs[1].type = MSK_BSDF_PLASTIC;
            mskscene::HostTables t6;
            CHECK(pack_one(s6, &t6) == MSK_OK, "pack");
            CHECK(word(t6.bsdfs, r + 5) == word(t.bsdfs, r + 20) && word(t6.bsdfs, r + 6) == word(t.bsdfs, r + 21), "type 6 and type 7 compute the same constants");
            for (int k = 1; k < 28; ++k)
                if (k != 5 && k != 6 && k != 20 && k != 21) CHECK(word(t6.bsdfs, r + k) == word(t.bsdfs, r + k), "word %d differs between type 6 and type 7", k);
            CHECK(t6.bsdfs.size() == t.bsdfs.size() && !std::memcmp(&t6.bsdfs[r + 28], &t.bsdfs[r + 28], (t.bsdfs.size() - r - 28) * 4), "everything behind the record");
            // the other entries' records, and the texture records, are those of the scene with a diffuse entry 1
            Scene s0; make(s0, false);
            mskscene::HostTables t0;
            CHECK(pack_one(s0, &t0) == MSK_OK, "pack");
            CHECK(t.mask_base == t0.n_bsdf_f4 && t.n_bsdf_f4 == t0.n_bsdf_f4 + 9u && t.bsdfs.size() == (size_t) t.n_bsdf_f4 * 4, "mask records: base %u", t.mask_base);
            CHECK(!std::memcmp(t.bsdfs.data(), t0.bsdfs.data(), 4 * MSK_BSDF_F4 * 4) && !std::memcmp(&t.bsdfs[8 * MSK_BSDF_F4], &t0.bsdfs[8 * MSK_BSDF_F4], (t0.bsdfs.size() - 8 * MSK_BSDF_F4) * 4), "records around the roughplastic changed");
            for (uint32_t e = 0; e < 3; ++e) {
                const size_t q = ((size_t) t.mask_base + 3u * e) * 4;
                for (int k = 0; k < 12; ++k) CHECK(word(t.bsdfs, q + k) == (k == 5 ? 0x3f800000u : 0u), "entry %u word %d: not {filter 0, opacity 1}", e, k);
            }
            // with a mask of its own: the mask's records and no others; with a lens on top: still one set
            msk_mask_desc m;
            std::memset(&m, 0, sizeof m);
            m.bsdf = 1; m.opacity = 0.25f;
            mskscene::HostTables tm;
            CHECK(pack_one(s, &tm, 1, &m) == MSK_OK, "pack");
            CHECK(tm.has_mask && tm.has_plastic && tm.n_bsdf_f4 == t.n_bsdf_f4 && tm.mask_base == t.mask_base && tm.bsdfs[((size_t) tm.mask_base + 4u) * 4 + 1] == 0.25f, "mask over roughplastic");
            CHECK(!std::memcmp(tm.bsdfs.data(), t.bsdfs.data(), (size_t) t.mask_base * 16), "a mask changed the roughplastic's record");
            mskscene::HostTables tl = t;
            mskscene::add_lens_tables(&s.d, &tl);
            CHECK(tl.n_bsdf_f4 == t.n_bsdf_f4 && tl.bsdfs.size() == t.bsdfs.size() && !std::memcmp(tl.bsdfs.data(), t.bsdfs.data(), t.bsdfs.size() * 4) && !tl.all_diffuse, "a lens added a second set of mask records");
        }
    std::printf("ok %d\n", n_checks);
    return 0;
}
