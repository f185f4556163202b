// light_tables_check.cpp — the `spot` / `directional` part of scene creation's host side on a CPU, for tests/test_spot_directional.py:
// what csrc/msk_scene_tables.h packs for msk_light_desc (the bytes of the two records), every refusal with its text, the radius a
// sun's scene gets, and that a scene without the new lights packs to the bytes it had through the older entry.  Stand-alone; built
// with and without -fsanitize=address,undefined.  Prints "ok <checks>" and returns 0, or the first failure and 1.
//   light_tables_check plan     csrc/msk_plan.h with the facts of a spot-only and of a sun-only scene as the packer states them, over
//                               the cross product of launch_plan_delta_check.cpp (knobs from the environment): every plan names
//                               SHADE_DELTA.  Prints "cases N".
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
static msk_emitter_desc emitter(int32_t type, int32_t mesh) {
    msk_emitter_desc e;
    std::memset(&e, 0, sizeof e);
    e.type = type; e.mesh_id = mesh; e.radiance[0] = 0.5f; e.radiance[1] = -0.25f; e.radiance[2] = 2.f; e.d65_scale = 0.015625f;
    return e;
}
// two quads and the emitters of `types` in order; an MSK_EMITTER_AREA entry lights the second quad
static void make(Scene &s, const std::vector<int32_t> &types) {
    std::memset(&s.d, 0, sizeof s.d);
    s.d.abi_version = MSK_ABI_VERSION;
    for (int i = 0; i < 3 * MSK_CIE_SAMPLES; ++i) s.cie[i] = 0.0078125f * (float) ((i * 37) % 101);
    for (int i = 0; i < MSK_CIE_SAMPLES; ++i) s.d65[i] = 40.f + 0.75f * (float) ((i * 11) % 64);
    for (int k = 0; k < 4; ++k) { s.d.camera.sample_to_camera[k * 5] = 1.f; s.d.camera.to_world[k * 5] = 1.f; }
    s.d.camera.near_clip = 0.01f; s.d.camera.far_clip = 100.f;
    s.d.film.width = 16; s.d.film.height = 8; s.d.film.filter_radius = 0.5f;
    for (int i = 0; i < MSK_FILTER_RESOLUTION; ++i) s.d.film.filter_lut[i] = 1.f;
    int area = -1;
    for (size_t k = 0; k < types.size(); ++k) {
        if (types[k] == MSK_EMITTER_AREA) area = (int) k;
        s.emitters.push_back(emitter(types[k], types[k] == MSK_EMITTER_AREA ? 1 : -1));
    }
    quad(s, 0.f, 0, -1); quad(s, 1.f, 1, area);
    s.bsdfs = {diffuse(0.25f), diffuse(0.f)};
    s.d.n_meshes = (uint32_t) s.meshes.size(); s.d.meshes = s.meshes.data();
    s.d.n_bsdfs = (uint32_t) s.bsdfs.size(); s.d.bsdfs = s.bsdfs.data();
    s.d.n_emitters = (uint32_t) s.emitters.size(); s.d.emitters = s.emitters.empty() ? nullptr : s.emitters.data();
    s.d.n_vertices = (uint32_t) (s.vertices.size() / 8); s.d.vertices = s.vertices.data();
    s.d.n_faces = (uint32_t) (s.faces.size() / 3); s.d.faces = s.faces.data();
    s.d.cie1931_xyz = s.cie; s.d.d65 = s.d65;
}
static msk_light_desc light(uint32_t e, float px, float py, float pz, float dx, float dy, float dz, float cc, float cb) {
    msk_light_desc l;
    std::memset(&l, 0, sizeof l);
    l.emitter = e; l.position[0] = px; l.position[1] = py; l.position[2] = pz; l.direction[0] = dx; l.direction[1] = dy; l.direction[2] = dz;
    l.cos_cutoff = cc; l.cos_beam = cb;
    return l;
}
static uint32_t word(const std::vector<float> &v, size_t i) { uint32_t w; std::memcpy(&w, &v[i], 4); return w; }
static bool same(const std::vector<float> &a, const std::vector<float> &b) { return a.size() == b.size() && (a.empty() || !std::memcmp(a.data(), b.data(), a.size() * 4)); }

// the scene {area, spot, directional} with `lights`, refused with `words`
static int refusal(const char *name, uint32_t n, const msk_light_desc *ptr, const char *words, int mesh_of_1 = -1) {
    Scene s; make(s, {MSK_EMITTER_AREA, MSK_EMITTER_SPOT, MSK_EMITTER_DIRECTIONAL});
    s.emitters[1].mesh_id = mesh_of_1;
    mskscene::HostTables t; std::string msg;
    const int rc = mskscene::pack(&s.d, nullptr, nullptr, &t, &msg, 0, nullptr, n, ptr);
    CHECK(rc == MSK_ERR_INVALID_ARG, "%s: code %d, message \"%s\"", name, rc, msg.c_str());
    CHECK(msg.find(words) != std::string::npos, "%s: \"%s\" does not say \"%s\"", name, msg.c_str(), words);
    CHECK(msg.find("emitter ") != std::string::npos || msg.find("msk_light_desc ") != std::string::npos || msg.find("n_lights") != std::string::npos,
          "%s: \"%s\" names neither the emitter nor the descriptor", name, msg.c_str());
    return 0;
}

static int plan_check() {
    using namespace mskplan;
    const RenderKnobs knobs = read_render_knobs();
    static const size_t lds[7][2] = {{24576, 8192}, {53248, 8192}, {53264, 8192}, {24576, 65024}, {24576, 65040}, {24576, 40960}, {24576, 40976}};
    static const uint32_t region_sizes[4] = {256, 1024, 2048, 8192};
    unsigned long n = 0;
    for (int which = 0; which < 2; ++which) {
        Scene s; make(s, {which ? MSK_EMITTER_DIRECTIONAL : MSK_EMITTER_SPOT});
        const msk_light_desc l = light(0, 1.f, 4.f, 1.f, 0.f, -1.f, 0.f, 0.5f, 0.75f);
        mskscene::HostTables t; std::string msg;
        if (mskscene::pack(&s.d, nullptr, nullptr, &t, &msg, 0, nullptr, 1, &l) != MSK_OK) { std::printf("pack: %s\n", msg.c_str()); return 1; }
        if (!t.has_delta || t.all_diffuse || t.has_envmap || t.has_mask || t.env_emitter != -1) { std::printf("the packer's flags of a %s-only scene\n", which ? "sun" : "spot"); return 1; }
        for (int mode = 0; mode <= 6; ++mode)
            for (int flags = 0; flags < 4; ++flags)
                for (int aov = 0; aov < 4; ++aov)
                    for (uint32_t rs : region_sizes)
                        for (const auto &b : lds) {
                            SceneFacts f;
                            f.trace_mode = mode; f.lds_scene = mode == TRACE_BIN_LDS || mode == TRACE_WIDE4_LDS;
                            f.lds_tables = flags & 1; f.cull_ok = flags & 2;
                            f.all_diffuse = t.all_diffuse; f.has_regular = t.has_regular; f.has_dielectric = t.has_dielectric; f.has_bitmap = t.has_bitmap;
                            f.has_envmap = t.has_envmap; f.has_delta = t.has_delta; f.has_mask = t.has_mask;
                            f.shade_lds_bytes = b[0]; f.trace_lds_bytes = b[1];
                            CallFacts c;
                            c.region_size = rs; c.aov_groups = (aov & 1) ? 2u : 0u; c.aov_rgb = (aov & 2) != 0;
                            const LaunchPlan p = make_launch_plan(f, c, knobs);
                            if (p.shade_kind != SHADE_DELTA || !p.dielectric || p.diffuse_only) {
                                std::printf("%s-only scene: shade_kind %d (SHADE_DELTA is %d): mode %d flags %d aov %d region_size %u\n", which ? "sun" : "spot", (int) p.shade_kind,
                                            (int) SHADE_DELTA, mode, flags, aov, rs);
                                return 1;
                            }
                            ++n;
                        }
    }
    std::printf("cases %lu\n", n);
    return 0;
}

int main(int argc, char **argv) {
    if (argc > 1 && std::string(argv[1]) == "plan") return plan_check();
    static_assert(sizeof(msk_light_desc) == 36 && offsetof(msk_light_desc, position) == 4 && offsetof(msk_light_desc, direction) == 16 &&
                      offsetof(msk_light_desc, cos_cutoff) == 28 && offsetof(msk_light_desc, cos_beam) == 32, "msk_light_desc layout");
    static_assert(sizeof(msk_scene_lights) == sizeof(msk_scene_masks) + 16 && offsetof(msk_scene_lights, n_lights) == sizeof(msk_scene_masks), "msk_scene_lights layout");
    static_assert(MSK_EMITTER_SPOT == 4 && MSK_EMITTER_DIRECTIONAL == 5 && MSK_ABI_VERSION == 8, "constants");
    std::string msg;
    // ---- a scene without the new lights packs to the same bytes through the old and the new entry
    {
        Scene s; make(s, {MSK_EMITTER_AREA, MSK_EMITTER_POINT, MSK_EMITTER_CONSTANT});
        const msk_point_desc pd = {1, {1.f, 2.f, 3.f}};
        const msk_scene_ext ext = {nullptr, 1, &pd};
        mskscene::HostTables a, b;
        CHECK(mskscene::pack(&s.d, &ext, nullptr, &a, &msg) == MSK_OK, "%s", msg.c_str());
        CHECK(mskscene::pack(&s.d, &ext, nullptr, &b, &msg, 0, nullptr, 0, nullptr) == MSK_OK, "%s", msg.c_str());
        CHECK(same(a.emitters, b.emitters) && same(a.cdf_all, b.cdf_all) && same(a.d65, b.d65) && same(a.emitter_grid, b.emitter_grid) && same(a.bsdfs, b.bsdfs) &&
                  same(a.tv, b.tv) && same(a.texels, b.texels), "no lights: tables differ");
        CHECK(a.env_radius == b.env_radius && a.env_emitter == b.env_emitter && a.has_delta == b.has_delta && a.all_diffuse == b.all_diffuse, "no lights: flags");
        CHECK(a.cdf_all.size() == 3u, "the area emitter's CDF alone: %zu", a.cdf_all.size());
        // a light descriptor that no emitter asks for is refused, not ignored
        const msk_light_desc l = light(1, 0, 0, 0, 0, 1, 0, 0.f, 0.5f);
        mskscene::HostTables c;
        CHECK(mskscene::pack(&s.d, &ext, nullptr, &c, &msg, 0, nullptr, 1, &l) == MSK_ERR_INVALID_ARG && msg.find("msk_light_desc 0: emitter 1 is of type 3") != std::string::npos, "%s", msg.c_str());
    }
    // ---- the bytes of the two records: {area, spot, directional, spot}, descriptors in another order
    {
        Scene s; make(s, {MSK_EMITTER_AREA, MSK_EMITTER_SPOT, MSK_EMITTER_DIRECTIONAL, MSK_EMITTER_SPOT});
        const msk_light_desc ls[3] = {light(3, -1.f, 0.5f, 8.f, 0.6f, 0.f, -0.8f, -1.f, -1.f), light(2, 9.f, 9.f, 9.f, 0.f, -0.6f, 0.8f, 7.f, -3.f),
                                      light(1, 1.5f, 4.f, -2.f, 0.f, -1.f, 0.f, 0.25f, 0.75f)};
        mskscene::HostTables t;
        CHECK(mskscene::pack(&s.d, nullptr, nullptr, &t, &msg, 0, nullptr, 3, ls) == MSK_OK, "%s", msg.c_str());
        CHECK(t.has_delta && !t.all_diffuse && t.env_emitter == -1 && !t.has_envmap, "flags");
        CHECK(t.emitters.size() == 4u * 8u && t.cdf_all.size() == 3u + 5u + 5u, "sizes %zu %zu", t.emitters.size(), t.cdf_all.size());
        CHECK((std::vector<int32_t>{0, 4, 5, 4}) == t.emitter_types, "emitter_types");
        // the spot, emitter 1: {c0, c1, c2, offset bits} {MARK_SPOT, position}; its five floats at the offset
        CHECK(t.emitters[8] == 0.5f && t.emitters[9] == -0.25f && t.emitters[10] == 2.f && word(t.emitters, 11) == 3u, "spot 1, first float4 (offset %u)", word(t.emitters, 11));
        CHECK(word(t.emitters, 12) == MSK_EMITTER_MARK_SPOT && t.emitters[13] == 1.5f && t.emitters[14] == 4.f && t.emitters[15] == -2.f, "spot 1, second float4");
        const float want1[5] = {0.f, -1.f, 0.f, 0.25f, 0.75f}, want3[5] = {0.6f, 0.f, -0.8f, -1.f, -1.f};
        CHECK(!std::memcmp(&t.cdf_all[3], want1, 20), "spot 1, pool");
        CHECK(word(t.emitters, 27) == 8u && word(t.emitters, 28) == MSK_EMITTER_MARK_SPOT && t.emitters[29] == -1.f && t.emitters[30] == 0.5f && t.emitters[31] == 8.f, "spot 3, record");
        CHECK(!std::memcmp(&t.cdf_all[8], want3, 20), "spot 3, pool");
        // the sun, emitter 2: {c0, c1, c2, 0} {MARK_DIRECTIONAL, -direction}; position and cosines ignored
        CHECK(word(t.emitters, 19) == 0u && word(t.emitters, 20) == MSK_EMITTER_MARK_DIRECTIONAL, "sun, marks");
        CHECK(word(t.emitters, 21) == 0x80000000u && t.emitters[22] == 0.6f && t.emitters[23] == -0.8f, "sun, d = -direction to the bit (-0 for +0)");
        // the area emitter in front of them is what it is without them
        Scene s0; make(s0, {MSK_EMITTER_AREA});
        mskscene::HostTables t0;
        CHECK(mskscene::pack(&s0.d, nullptr, nullptr, &t0, &msg) == MSK_OK, "%s", msg.c_str());
        CHECK(!std::memcmp(t.emitters.data(), t0.emitters.data(), 32) && !std::memcmp(t.cdf_all.data(), t0.cdf_all.data(), 12), "the area emitter's record changed");
        CHECK(t0.env_radius == 0.f, "a scene without environment or sun has no radius");
        CHECK(MSK_EMITTER_MARK_DELTA_FIRST == MSK_EMITTER_MARK_DIRECTIONAL && MSK_EMITTER_MARK_SPOT == MSK_EMITTER_MARK_DIRECTIONAL + 1u &&
                  MSK_EMITTER_MARK_POINT == MSK_EMITTER_MARK_SPOT + 1u, "the three marks are consecutive");
    }
    // ---- a sun alone gets the radius the same scene gets with a `constant` sky, and keeps env_emitter
    {
        Scene a; make(a, {MSK_EMITTER_DIRECTIONAL});
        Scene b; make(b, {MSK_EMITTER_CONSTANT});
        const msk_light_desc l = light(0, 0, 0, 0, 0.f, -1.f, 0.f, 0.f, 0.f);
        mskscene::HostTables ta, tb;
        CHECK(mskscene::pack(&a.d, nullptr, nullptr, &ta, &msg, 0, nullptr, 1, &l) == MSK_OK, "%s", msg.c_str());
        CHECK(mskscene::pack(&b.d, nullptr, nullptr, &tb, &msg) == MSK_OK, "%s", msg.c_str());
        CHECK(ta.env_radius > 0.f && ta.env_radius == tb.env_radius, "radius %g vs %g", (double) ta.env_radius, (double) tb.env_radius);
        CHECK(ta.env_emitter == -1 && tb.env_emitter == 0, "env_emitter");
        Scene c; make(c, {MSK_EMITTER_SPOT});
        const msk_light_desc lc = light(0, 0, 3, 0, 0.f, -1.f, 0.f, 0.f, 0.5f);
        mskscene::HostTables tc;
        CHECK(mskscene::pack(&c.d, nullptr, nullptr, &tc, &msg, 0, nullptr, 1, &lc) == MSK_OK, "%s", msg.c_str());
        CHECK(tc.env_radius == 0.f && tc.has_delta, "a spot needs no radius");
    }
    // ---- every refusal, with its text.  The scene: {area, spot (1), directional (2)}
    const msk_light_desc spot = light(1, 1.f, 4.f, 1.f, 0.f, -1.f, 0.f, 0.5f, 0.75f), sun = light(2, 0, 0, 0, 0.6f, -0.8f, 0.f, 0.f, 0.f);
    {   // the pair itself is fine, in either order
        Scene s; make(s, {MSK_EMITTER_AREA, MSK_EMITTER_SPOT, MSK_EMITTER_DIRECTIONAL});
        const msk_light_desc a[2] = {spot, sun}, b[2] = {sun, spot};
        mskscene::HostTables ta, tb;
        CHECK(mskscene::pack(&s.d, nullptr, nullptr, &ta, &msg, 0, nullptr, 2, a) == MSK_OK, "%s", msg.c_str());
        CHECK(mskscene::pack(&s.d, nullptr, nullptr, &tb, &msg, 0, nullptr, 2, b) == MSK_OK, "%s", msg.c_str());
        CHECK(same(ta.emitters, tb.emitters) && same(ta.cdf_all, tb.cdf_all), "the order of the descriptors changes the tables");
    }
    { if (refusal("no descriptors", 0, nullptr, "emitter 1: a spot emitter needs its geometry")) return 1; }
    { const msk_light_desc m[1] = {spot}; if (refusal("sun missing", 1, m, "emitter 2: a directional emitter needs its geometry")) return 1; }
    { const msk_light_desc m[1] = {sun}; if (refusal("spot missing", 1, m, "emitter 1: a spot emitter needs its geometry")) return 1; }
    { const msk_light_desc m[3] = {spot, sun, spot}; if (refusal("spot twice", 3, m, "emitter 1: a spot emitter with two descriptors (msk_light_desc 2 is its second)")) return 1; }
    { const msk_light_desc m[3] = {spot, sun, sun}; if (refusal("sun twice", 3, m, "emitter 2: a directional emitter with two descriptors (msk_light_desc 2 is its second)")) return 1; }
    { msk_light_desc m[3] = {spot, sun, spot}; m[2].emitter = 0; if (refusal("other type", 3, m, "msk_light_desc 2: emitter 0 is of type 0, neither a spot (type 4) nor a directional emitter (type 5)")) return 1; }
    { msk_light_desc m[3] = {spot, sun, spot}; m[2].emitter = 7; if (refusal("range", 3, m, "msk_light_desc 2: emitter 7 out of range (the scene has 3)")) return 1; }
    { if (refusal("null lights", 2, nullptr, "msk_scene_lights: n_lights 2 without lights")) return 1; }
    for (float bad : {INFINITY, -INFINITY, NAN}) {
        for (int k = 0; k < 3; ++k) {
            msk_light_desc m[2] = {spot, sun}; m[0].position[k] = bad;
            if (refusal("position", 2, m, "emitter 1: a spot emitter's position must be finite")) return 1;
            msk_light_desc q[2] = {spot, sun}; q[0].direction[k] = bad;
            if (refusal("spot direction", 2, q, "emitter 1: a spot emitter's direction must be finite")) return 1;
            msk_light_desc r[2] = {spot, sun}; r[1].direction[k] = bad;
            if (refusal("sun direction", 2, r, "emitter 2: a directional emitter's direction must be finite")) return 1;
        }
        msk_light_desc m[2] = {spot, sun}; m[1].position[0] = bad;          // a sun's position is ignored
        Scene s; make(s, {MSK_EMITTER_AREA, MSK_EMITTER_SPOT, MSK_EMITTER_DIRECTIONAL});
        mskscene::HostTables t;
        CHECK(mskscene::pack(&s.d, nullptr, nullptr, &t, &msg, 0, nullptr, 2, m) == MSK_OK, "%s", msg.c_str());
    }
    { msk_light_desc m[2] = {spot, sun}; m[0].direction[1] = -1.00002f; if (refusal("long axis", 2, m, "emitter 1: a spot emitter's direction must have unit length")) return 1; }
    { msk_light_desc m[2] = {spot, sun}; m[1].direction[0] = 0.f; m[1].direction[1] = 0.f; if (refusal("zero sun", 2, m, "emitter 2: a directional emitter's direction must have unit length")) return 1; }
    { msk_light_desc m[2] = {spot, sun}; m[1].direction[1] = -0.79f; if (refusal("short sun", 2, m, "emitter 2: a directional emitter's direction must have unit length")) return 1; }
    { msk_light_desc m[2] = {spot, sun}; m[0].cos_cutoff = 1.f; m[0].cos_beam = 1.f; if (refusal("cutoff 1", 2, m, "emitter 1: a spot emitter's cos_cutoff 1 is outside [-1, 1)")) return 1; }
    { msk_light_desc m[2] = {spot, sun}; m[0].cos_cutoff = -1.5f; if (refusal("cutoff below", 2, m, "emitter 1: a spot emitter's cos_cutoff -1.5 is outside [-1, 1)")) return 1; }
    { msk_light_desc m[2] = {spot, sun}; m[0].cos_cutoff = NAN; if (refusal("cutoff nan", 2, m, "is outside [-1, 1)")) return 1; }
    { msk_light_desc m[2] = {spot, sun}; m[0].cos_beam = 0.25f; if (refusal("beam below the cutoff", 2, m, "emitter 1: a spot emitter's cos_beam 0.25 is outside [cos_cutoff, 1] (cos_cutoff 0.5)")) return 1; }
    { msk_light_desc m[2] = {spot, sun}; m[0].cos_beam = 1.25f; if (refusal("beam above 1", 2, m, "emitter 1: a spot emitter's cos_beam 1.25 is outside [cos_cutoff, 1]")) return 1; }
    { msk_light_desc m[2] = {spot, sun}; m[0].cos_beam = NAN; if (refusal("beam nan", 2, m, "is outside [cos_cutoff, 1]")) return 1; }
    { const msk_light_desc m[2] = {spot, sun}; if (refusal("mesh", 2, m, "emitter 1: a spot emitter has no mesh (mesh_id must be -1)", 0)) return 1; }
    {   // ... and the sun's
        Scene s; make(s, {MSK_EMITTER_AREA, MSK_EMITTER_SPOT, MSK_EMITTER_DIRECTIONAL});
        s.emitters[2].mesh_id = 0;
        const msk_light_desc m[2] = {spot, sun};
        mskscene::HostTables t;
        CHECK(mskscene::pack(&s.d, nullptr, nullptr, &t, &msg, 0, nullptr, 2, m) == MSK_ERR_INVALID_ARG && msg.find("emitter 2: a directional emitter has no mesh (mesh_id must be -1)") != std::string::npos, "%s", msg.c_str());
    }
    {   // the limits themselves are taken: cos_cutoff -1, cos_beam == cos_cutoff, cos_beam 1, a squared length 1e-5 off
        Scene s; make(s, {MSK_EMITTER_AREA, MSK_EMITTER_SPOT, MSK_EMITTER_DIRECTIONAL});
        msk_light_desc m[2] = {spot, sun};
        mskscene::HostTables t;
        m[0].cos_cutoff = -1.f; m[0].cos_beam = -1.f;
        CHECK(mskscene::pack(&s.d, nullptr, nullptr, &t, &msg, 0, nullptr, 2, m) == MSK_OK, "%s", msg.c_str());
        m[0].cos_cutoff = 0.5f; m[0].cos_beam = 1.f;
        CHECK(mskscene::pack(&s.d, nullptr, nullptr, &t, &msg, 0, nullptr, 2, m) == MSK_OK, "%s", msg.c_str());
        m[0].direction[1] = -1.000004f;
        CHECK(mskscene::pack(&s.d, nullptr, nullptr, &t, &msg, 0, nullptr, 2, m) == MSK_OK, "%s", msg.c_str());
    }
    // ---- an unknown type keeps its words
    {
        Scene s; make(s, {MSK_EMITTER_AREA, 9});
        mskscene::HostTables t;
        CHECK(mskscene::pack(&s.d, nullptr, nullptr, &t, &msg) == MSK_ERR_UNSUPPORTED && msg == "emitter 1: type 9 is not supported (area, constant, envmap, point)", "%s", msg.c_str());
    }
    std::printf("ok %d\n", n_checks);
    return 0;
}
