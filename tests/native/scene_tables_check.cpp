// scene_tables_check.cpp — scene creation's host side on a CPU, for tests/test_scene_tables.py: what csrc/msk_scene_tables.h
// refuses and packs, and where csrc/msk_plan.h places tree and tables.  Knobs come from the environment, through
// read_scene_knobs(), as in msk_gpu_scene_create.
//   scene_tables_check refusals     "name code message" per case: a descriptor that is valid but for one field (or, "two_*", two)
//   scene_tables_check tables       per built-in descriptor "scene name", then "key values..." lines: flags, counts, the integer
//                                   words of the records, and per vector "vec name length fnv1a-64 of its bytes"
//   scene_tables_check placement    "tree ..." per case of the tree cross product and "sizes ..." per set of counts: inputs | outcome
#include "../../misaki-render_amd/csrc/msk_scene_tables.h"
#include "../../misaki-render_amd/csrc/msk_plan.h"

#include <cstdio>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

// ----------------------------------------------------------------------------- descriptors
struct Scene {
    std::vector<msk_mesh_desc> meshes;
    std::vector<msk_bsdf_desc> bsdfs;
    std::vector<msk_emitter_desc> emitters;
    std::vector<float> vertices;
    std::vector<uint32_t> faces;
    std::vector<msk_texture_desc> textures;
    std::vector<msk_regular_spectrum_desc> regular;
    std::vector<float> regular_values, texels, env_texels, env_weights;
    std::vector<msk_point_desc> points;
    float cie[3 * MSK_CIE_SAMPLES], d65[MSK_CIE_SAMPLES];
    msk_envmap_desc env;
    bool with_env = false, with_ext = false;
    msk_scene_ext ext;
    msk_scene_desc d;

    // counts and pointers of the descriptor from the vectors (an empty vector gives a null pointer)
    void link() {
        auto ptr = [](auto &v) { return v.empty() ? nullptr : v.data(); };
        d.n_meshes = (uint32_t) meshes.size(); d.meshes = ptr(meshes);
        d.n_bsdfs = (uint32_t) bsdfs.size(); d.bsdfs = ptr(bsdfs);
        d.n_emitters = (uint32_t) emitters.size(); d.emitters = ptr(emitters);
        d.n_vertices = (uint32_t) (vertices.size() / 8); d.vertices = ptr(vertices);
        d.n_faces = (uint32_t) (faces.size() / 3); d.faces = ptr(faces);
        d.n_textures = (uint32_t) textures.size(); d.textures = ptr(textures);
        d.n_regular_spectra = (uint32_t) regular.size(); d.regular_spectra = ptr(regular);
        d.n_regular_values = (uint32_t) regular_values.size(); d.regular_values = ptr(regular_values);
        d.n_texels = (uint32_t) (texels.size() / 3); d.texels = ptr(texels);
        d.cie1931_xyz = cie; d.d65 = d65;
        env.texels = ptr(env_texels); env.weights = ptr(env_weights);
        ext.envmap = with_env ? &env : nullptr; ext.n_points = (uint32_t) points.size(); ext.points = ptr(points);
    }
    const msk_scene_ext *ext_ptr() const { return with_env || with_ext || !points.empty() ? &ext : nullptr; }
};

static msk_spectrum_desc spectrum(float c0, float c1, float c2, float scale) {
    msk_spectrum_desc s;
    std::memset(&s, 0, sizeof s);
    s.coeff[0] = c0; s.coeff[1] = c1; s.coeff[2] = c2; s.scale = scale;
    return s;
}
static msk_bsdf_desc diffuse(float c0, float c1, float c2) {
    msk_bsdf_desc b;
    std::memset(&b, 0, sizeof b);
    b.type = MSK_BSDF_DIFFUSE; b.back_bsdf = -1;
    b.reflectance[0] = c0; b.reflectance[1] = c1; b.reflectance[2] = c2; b.reflectance_scale = 1.f;
    b.eta = b.k = spectrum(0.f, 0.f, INFINITY, 1.f);
    b.specular_reflectance = b.specular_transmittance = spectrum(0.f, 0.f, INFINITY, 1.f);
    b.ior_eta = 1.5f; b.ior_inv_eta = 1.f / 1.5f;
    return b;
}
static msk_emitter_desc emitter(int32_t type, int32_t mesh) {
    msk_emitter_desc e;
    std::memset(&e, 0, sizeof e);
    e.type = type; e.mesh_id = mesh;
    e.radiance[0] = 0.5f; e.radiance[1] = -1.25f; e.radiance[2] = 2.f; e.d65_scale = 0.015625f;
    return e;
}
static void quad(Scene &s, float y, float lo, float hi, bool up, int32_t bsdf, int32_t em) {
    msk_mesh_desc m;
    std::memset(&m, 0, sizeof m);
    m.first_vertex = (uint32_t) (s.vertices.size() / 8); m.vertex_count = 4;
    m.first_face = (uint32_t) (s.faces.size() / 3); m.face_count = 2;
    m.bsdf_id = bsdf; m.emitter_id = em;
    const float p[4][2] = {{lo, lo}, {hi, lo}, {hi, hi}, {lo, hi}};
    for (int k = 0; k < 4; ++k) {
        const float v[8] = {p[k][0], y, p[k][1], 0.f, up ? 1.f : -1.f, 0.f, p[k][0] * 0.5f + 0.125f, p[k][1] * 0.25f};
        s.vertices.insert(s.vertices.end(), v, v + 8);
    }
    const uint32_t f_up[6] = {0, 2, 1, 0, 3, 2}, f_down[6] = {0, 1, 2, 0, 2, 3};
    s.faces.insert(s.faces.end(), up ? f_up : f_down, (up ? f_up : f_down) + 6);
    s.meshes.push_back(m);
}

static const char *kScenes[8] = {"quad", "bitmap", "checkerboard", "regular", "envmap", "point_conductor", "constant_sky", "zero_faces"};

// a lit quad under an emitter quad: 4 triangles, 2 meshes, one area emitter — and what each name adds to it
static void make(const std::string &name, Scene &s) {
    std::memset(&s.d, 0, sizeof s.d); std::memset(&s.env, 0, sizeof s.env); std::memset(&s.ext, 0, sizeof s.ext);
    s.d.abi_version = MSK_ABI_VERSION;
    for (int i = 0; i < 3 * MSK_CIE_SAMPLES; ++i) s.cie[i] = 0.0078125f * (float) ((i * 37) % 101);
    for (int i = 0; i < MSK_CIE_SAMPLES; ++i) s.d65[i] = 40.f + 0.75f * (float) ((i * 11) % 64);
    for (int k = 0; k < 4; ++k) { s.d.camera.sample_to_camera[k * 5] = 1.f; s.d.camera.to_world[k * 5] = 1.f; }
    s.d.camera.near_clip = 0.01f; s.d.camera.far_clip = 100.f;
    s.d.film.width = 16; s.d.film.height = 8; s.d.film.filter_radius = 0.5f;
    for (int i = 0; i < MSK_FILTER_RESOLUTION; ++i) s.d.film.filter_lut[i] = 1.f;
    if (name == "zero_faces") {
        msk_mesh_desc m;
        std::memset(&m, 0, sizeof m);
        m.emitter_id = -1;
        s.meshes.push_back(m);
        s.bsdfs.push_back(diffuse(0.25f, 0.5f, -0.75f));
        return;
    }
    quad(s, 0.f, 0.f, 1.f, true, 0, -1);
    quad(s, 1.f, 0.25f, 0.75f, false, 1, 0);
    s.bsdfs.push_back(diffuse(0.25f, 0.5f, -0.75f));
    s.bsdfs.push_back(diffuse(0.f, 0.f, 1.5f));
    s.emitters.push_back(emitter(MSK_EMITTER_AREA, 1));
    if (name == "bitmap" || name == "checkerboard") {
        msk_texture_desc t;
        std::memset(&t, 0, sizeof t);
        t.type = name == "bitmap" ? MSK_TEXTURE_BITMAP : MSK_TEXTURE_CHECKERBOARD;
        t.color0[0] = 0.5f; t.color0[1] = 1.f; t.color0[2] = -2.f; t.color1[0] = -0.5f; t.color1[1] = 0.25f; t.color1[2] = 3.f;
        const float to_uv[6] = {4.f, 0.5f, 0.125f, -0.25f, 3.f, 0.75f};
        std::memcpy(t.to_uv, to_uv, sizeof to_uv);
        if (name == "bitmap") {
            t.width = 2; t.height = 2; t.first_texel = 0;
            for (int i = 0; i < 12; ++i) s.texels.push_back(0.125f * (float) (i - 5));
            s.meshes[0].has_normals = 1;
        }
        s.meshes[0].has_texcoords = 1;
        s.textures.push_back(t);
        s.bsdfs[0].reflectance_texture = 1;
    } else if (name == "regular") {
        s.regular.push_back({400.f, 700.f, 5u, 0u});
        s.regular.push_back({360.f, 830.f, 3u, 5u});
        for (float v : {0.25f, 0.5f, 0.75f, 0.5f, 0.125f, 2.f, 0.f, 4.f}) s.regular_values.push_back(v);
        s.bsdfs[0].reflectance_regular = 1;
        s.emitters[0].radiance_regular = 2;
    } else if (name == "envmap") {
        msk_emitter_desc e = emitter(MSK_EMITTER_ENVMAP, -1);
        e.radiance[0] = 0.f; e.radiance[1] = 0.f; e.radiance[2] = INFINITY; e.d65_scale = 1.f / 10568.f;
        s.emitters.push_back(e);
        s.with_env = true;
        s.env.width = 4; s.env.height = 2;
        for (int i = 0; i < 8; ++i) {
            const float t[4] = {0.25f * (float) i, -0.5f, 1.f + (float) i, i == 3 ? 0.f : 0.5f * (float) (i + 1)};
            s.env_texels.insert(s.env_texels.end(), t, t + 4);
            s.env_weights.push_back(i == 3 ? 0.f : 0.25f + (float) ((i * 5) % 7));
        }
        const float rot[9] = {0.f, 0.f, 1.f, 0.f, 1.f, 0.f, -1.f, 0.f, 0.f};
        std::memcpy(s.env.to_world, rot, sizeof rot);
    } else if (name == "point_conductor") {
        s.emitters.push_back(emitter(MSK_EMITTER_POINT, -1));
        s.points.push_back({1u, {0.5f, 0.75f, 0.25f}});
        msk_bsdf_desc &b = s.bsdfs[0];
        b.type = MSK_BSDF_CONDUCTOR; b.back_bsdf = 0; b.ior_eta = 1.f; b.ior_inv_eta = 1.f;
        b.eta = spectrum(0.f, 0.f, INFINITY, 0.2f); b.k = spectrum(0.f, 0.f, INFINITY, 3.9f);
    } else if (name == "constant_sky") {
        s.emitters.insert(s.emitters.begin(), emitter(MSK_EMITTER_CONSTANT, -1));      // the sky first: the area emitter becomes emitter 1
        s.emitters[1].mesh_id = 1; s.meshes[1].emitter_id = 1;
    }
}

// ----------------------------------------------------------------------------- refusals
struct Case { const char *name, *scene; std::function<void(Scene &)> mutate; const char *pad_scale; };

static std::vector<Case> refusal_cases() {
    const float nan = std::nanf("");
    auto tex_pool_missing = [](Scene &s) { s.d.texels = nullptr; };
    std::vector<Case> c = {
        // the descriptor's head
        {"abi_version", "quad", [](Scene &s) { s.d.abi_version = 7; }, nullptr},
        {"film", "quad", [](Scene &s) { s.d.film.filter_radius = 0.f; }, nullptr},
        {"crop", "quad", [](Scene &s) { s.d.film.crop_offset[0] = 9; s.d.film.crop_size[0] = 8; s.d.film.crop_size[1] = 8; }, nullptr},
        {"spectral_tables", "quad", [](Scene &s) { s.d.d65 = nullptr; }, nullptr},
        {"geometry_arrays", "quad", [](Scene &s) { s.d.faces = nullptr; }, nullptr},
        {"bsdf_emitter_arrays", "quad", [](Scene &s) { s.d.emitters = nullptr; }, nullptr},
        {"too_many_triangles", "quad", [](Scene &s) { s.d.n_faces = 1u << 26; }, nullptr},
        // meshes and triangles
        {"mesh_range", "quad", [](Scene &s) { s.meshes[1].face_count = 3; }, nullptr},
        {"mesh_bsdf_id", "quad", [](Scene &s) { s.meshes[0].bsdf_id = 2; }, nullptr},
        {"mesh_emitter_id", "quad", [](Scene &s) { s.meshes[0].emitter_id = 1; }, nullptr},
        {"mesh_emitter_back", "quad", [](Scene &s) { s.meshes[0].emitter_id = 0; }, nullptr},
        {"face_in_two_meshes", "quad", [](Scene &s) { s.meshes[1].first_face = 1; s.meshes[1].face_count = 1; }, nullptr},
        {"vertex_index", "quad", [](Scene &s) { s.faces[4] = 4; }, nullptr},
        {"vertex_not_finite", "quad", [](Scene &s) { s.vertices[8 * 5 + 1] = INFINITY; }, nullptr},
        {"face_in_no_mesh", "quad", [](Scene &s) { s.meshes[1].first_face = 3; s.meshes[1].face_count = 1; }, nullptr},
        // tabulated spectra
        {"regular_arrays", "regular", [](Scene &s) { s.d.regular_values = nullptr; }, nullptr},
        {"regular_too_many_values", "regular", [](Scene &s) { s.d.n_regular_values = 1u << 24; }, nullptr},
        {"regular_one_entry", "regular", [](Scene &s) { s.regular[1].size = 1; }, nullptr},
        {"regular_too_long", "regular", [](Scene &s) { s.regular[1].size = 96; }, nullptr},
        {"regular_range", "regular", [](Scene &s) { s.regular[0].lambda_max = 400.f; }, nullptr},
        {"regular_values_exceed", "regular", [](Scene &s) { s.regular[1].first_value = 6; }, nullptr},
        {"regular_negative", "regular", [](Scene &s) { s.regular_values[2] = -0.5f; }, nullptr},
        {"regular_no_mass", "regular", [](Scene &s) { s.regular_values[5] = 0.f; s.regular_values[7] = 0.f; }, nullptr},
        {"spectrum_names_regular", "regular", [](Scene &s) { s.bsdfs[1].eta.regular = 3; }, nullptr},
        {"spectrum_scale", "quad", [](Scene &s) { s.bsdfs[1].k.scale = -1.f; }, nullptr},
        // textures
        {"texture_array", "checkerboard", [](Scene &s) { s.d.textures = nullptr; }, nullptr},
        {"texture_type", "checkerboard", [](Scene &s) { s.textures[0].type = 7; }, nullptr},
        {"bitmap_size", "bitmap", [](Scene &s) { s.textures[0].height = 0; }, nullptr},
        {"bitmap_past_pool", "bitmap", [](Scene &s) { s.textures[0].first_texel = 1; }, nullptr},
        {"bitmap_pool_missing", "bitmap", tex_pool_missing, nullptr},
        {"bitmap_nan", "bitmap", [nan](Scene &s) { s.texels[7] = nan; }, nullptr},
        // BSDFs
        {"bsdf_type", "quad", [](Scene &s) { s.bsdfs[1].type = 5; }, nullptr},
        {"bsdf_back", "quad", [](Scene &s) { s.bsdfs[1].back_bsdf = 2; }, nullptr},
        {"bsdf_roughness", "quad", [](Scene &s) { s.bsdfs[1].type = MSK_BSDF_ROUGHCONDUCTOR; s.bsdfs[1].alpha_v = -0.1f; }, nullptr},
        {"bsdf_ior", "quad", [](Scene &s) { s.bsdfs[1].type = MSK_BSDF_ROUGHDIELECTRIC; s.bsdfs[1].ior_inv_eta = 0.f; }, nullptr},
        {"dielectric_nested", "quad", [](Scene &s) { s.bsdfs[1].type = MSK_BSDF_DIELECTRIC; s.bsdfs[1].back_bsdf = 1; }, nullptr},
        {"conductor_with_ior", "quad", [](Scene &s) { s.bsdfs[1].type = MSK_BSDF_CONDUCTOR; }, nullptr},
        {"bsdf_texture_range", "checkerboard", [](Scene &s) { s.bsdfs[0].reflectance_texture = 2; }, nullptr},
        {"bsdf_reflectance_scale", "quad", [](Scene &s) { s.bsdfs[1].reflectance_scale = INFINITY; }, nullptr},
        {"bsdf_textured_not_diffuse", "checkerboard", [](Scene &s) { s.bsdfs[0].type = MSK_BSDF_ROUGHCONDUCTOR; }, nullptr},
        {"bsdf_regular_and_texture", "checkerboard", [](Scene &s) { s.bsdfs[0].reflectance_regular = 1; }, nullptr},
        // emitters
        {"envmap_without_image", "envmap", [](Scene &s) { s.ext.envmap = nullptr; }, nullptr},
        {"envmap_regular_radiance", "envmap", [](Scene &s) { s.emitters[1].radiance_regular = 1; }, nullptr},
        {"envmap_scale", "envmap", [](Scene &s) { s.emitters[1].d65_scale = -1.f; }, nullptr},
        {"two_environments", "constant_sky", [](Scene &s) { s.emitters.push_back(emitter(MSK_EMITTER_CONSTANT, -1)); s.link(); }, nullptr},
        {"environment_with_mesh", "constant_sky", [](Scene &s) { s.emitters[0].mesh_id = 0; }, nullptr},
        {"area_mesh_back", "quad", [](Scene &s) { s.emitters.push_back(emitter(MSK_EMITTER_AREA, 0)); s.link(); }, nullptr},
        {"area_mesh_without_faces", "quad", [](Scene &s) {
             msk_mesh_desc m = s.meshes[1];
             m.first_face = 4; m.face_count = 0; m.emitter_id = 1;
             s.meshes.push_back(m); s.emitters.push_back(emitter(MSK_EMITTER_AREA, 2)); s.link();
         }, nullptr},
        {"point_with_mesh", "point_conductor", [](Scene &s) { s.emitters[1].mesh_id = 0; }, nullptr},
        {"point_two_positions", "point_conductor", [](Scene &s) { s.points.push_back(s.points[0]); s.link(); }, nullptr},
        {"point_without_position", "point_conductor", [](Scene &s) { s.points.clear(); s.with_ext = true; s.link(); }, nullptr},
        {"point_not_finite", "point_conductor", [](Scene &s) { s.points[0].position[2] = INFINITY; }, nullptr},
        {"emitter_type", "quad", [](Scene &s) { s.emitters.push_back(emitter(9, -1)); s.link(); }, nullptr},
        {"emitter_names_regular", "regular", [](Scene &s) { s.emitters[0].radiance_regular = 3; }, nullptr},
        {"points_missing", "quad", [](Scene &s) { s.with_ext = true; s.link(); s.ext.n_points = 1; }, nullptr},
        {"point_desc_range", "point_conductor", [](Scene &s) { s.points.push_back({9u, {0.f, 0.f, 0.f}}); s.link(); }, nullptr},
        {"point_desc_not_a_point", "point_conductor", [](Scene &s) { s.points.push_back({0u, {0.f, 0.f, 0.f}}); s.link(); }, nullptr},
        // the envmap emitter's image
        {"image_without_envmap", "quad", [](Scene &s) { s.with_env = true; s.link(); }, nullptr},
        {"envmap_size", "envmap", [](Scene &s) { s.env.width = 0; }, nullptr},
        {"envmap_too_large", "envmap", [](Scene &s) { s.env.width = 1u << 14; s.env.height = 1u << 14; }, nullptr},
        {"envmap_arrays", "envmap", [](Scene &s) { s.env.weights = nullptr; }, nullptr},
        {"envmap_factor", "envmap", [](Scene &s) { s.env_texels[4 * 2 + 3] = -1.f; }, nullptr},
        {"envmap_nan", "envmap", [nan](Scene &s) { s.env_texels[4 * 5 + 1] = nan; }, nullptr},
        {"envmap_weights", "envmap", [](Scene &s) { s.env_weights[6] = -2.f; }, nullptr},
        {"envmap_rotation", "envmap", [](Scene &s) { s.env.to_world[0] = 0.5f; }, nullptr},
        {"envmap_pool_offsets", "envmap", [](Scene &s) { s.d.n_texels = 0x7fffffffu; }, nullptr},
        // the padding
        {"pad_scale", "quad", [](Scene &) {}, "1e-9"},
        {"pad_scale_garbage", "quad", [](Scene &) {}, "1e-5x"},
        // two faults: the earlier check's message
        {"two_abi_then_film", "quad", [](Scene &s) { s.d.abi_version = 7; s.d.film.width = 0; }, nullptr},
        {"two_mesh_then_bsdf", "quad", [](Scene &s) { s.meshes[0].bsdf_id = 2; s.bsdfs[1].type = 5; }, nullptr},
        {"two_regular_then_texture", "regular", [](Scene &s) { s.regular[1].size = 1; s.d.n_textures = 1; }, nullptr},
        {"two_texture_then_bsdf", "checkerboard", [](Scene &s) { s.textures[0].type = 7; s.bsdfs[1].back_bsdf = 2; }, nullptr},
        {"two_bsdf_then_emitter", "quad", [](Scene &s) { s.bsdfs[1].back_bsdf = 2; s.emitters[0].type = 9; }, nullptr},
        {"two_emitter_then_image", "envmap", [](Scene &s) { s.emitters[0].radiance_regular = 3; s.env.width = 0; }, nullptr},
        {"two_image_then_pad_scale", "envmap", [](Scene &s) { s.env.to_world[0] = 0.5f; }, "0"},
        {"two_first_bsdf_then_second", "quad", [](Scene &s) { s.bsdfs[0].reflectance_scale = -1.f; s.bsdfs[1].type = 5; }, nullptr},
    };
    return c;
}

static int refusals() {
    for (const Case &c : refusal_cases()) {
        Scene s;
        make(c.scene, s);
        s.link();
        c.mutate(s);
        mskscene::HostTables t;
        std::string msg = "-";
        const int rc = mskscene::pack(&s.d, s.ext_ptr(), c.pad_scale, &t, &msg);
        std::printf("%s %d %s\n", c.name, rc, msg.c_str());
    }
    return 0;
}

// ----------------------------------------------------------------------------- tables
template <class T> static void print_vec(const char *name, const std::vector<T> &v) {
    uint64_t h = 1469598103934665603ull;                              // FNV-1a, 64 bit
    const unsigned char *p = (const unsigned char *) v.data();
    for (size_t k = 0; k < v.size() * sizeof(T); ++k) { h ^= p[k]; h *= 1099511628211ull; }
    std::printf("vec %s %zu %016llx\n", name, v.size(), (unsigned long long) h);
}
static uint32_t word(const float *f) { uint32_t w; std::memcpy(&w, f, 4); return w; }

static int tables() {
    const mskplan::SceneKnobs knobs = mskplan::read_scene_knobs();
    for (const char *name : kScenes) {
        Scene s;
        make(name, s);
        s.link();
        mskscene::HostTables t;
        std::string msg;
        const int rc = mskscene::pack(&s.d, s.ext_ptr(), knobs.pad_scale, &t, &msg);
        std::printf("scene %s\n", name);
        if (rc) { std::printf("refused %d %s\n", rc, msg.c_str()); continue; }
        std::printf("flags all_diffuse=%d has_regular=%d has_dielectric=%d has_bitmap=%d has_envmap=%d has_delta=%d any_normals=%d any_uvs=%d\n", (int) t.all_diffuse,
                    (int) t.has_regular, (int) t.has_dielectric, (int) t.has_bitmap, (int) t.has_envmap, (int) t.has_delta, (int) t.any_normals, (int) t.any_uvs);
        std::printf("counts n_bsdf_f4=%u env_emitter=%d n_textures=%u tex_base=%u\n", t.n_bsdf_f4, t.env_emitter, t.n_textures, t.tex_base);
        std::printf("floats tri_pad=%.9g env_radius=%.9g lo=%.9g,%.9g,%.9g hi=%.9g,%.9g,%.9g\n", t.tri_pad, t.env_radius, t.scene_lo[0], t.scene_lo[1], t.scene_lo[2],
                    t.scene_hi[0], t.scene_hi[1], t.scene_hi[2]);
        std::printf("mesh_info");
        for (int32_t v : t.mesh_info) std::printf(" %d", v);
        std::printf("\ntri_mesh");
        for (uint32_t f = 0; f < s.d.n_faces; ++f) std::printf(" %u", word(&t.tv[(size_t) f * 12 + 3]));
        std::printf("\nbsdf_words");                                   // per BSDF: type, back_bsdf, sample_visible, texture offset
        for (uint32_t b = 0; b < s.d.n_bsdfs; ++b) {
            const float *o = &t.bsdfs[(size_t) b * 4 * MSK_BSDF_F4];
            std::printf(" %d,%d,%d,%u", (int32_t) word(&o[0]), (int32_t) word(&o[1]), (int32_t) word(&o[7]), word(&o[26]));
        }
        std::printf("\ntexture_words");                                // per texture: words 0, 1, 2 and 4 of its record
        for (uint32_t k = 0; k < t.n_textures; ++k) {
            const float *o = &t.bsdfs[((size_t) t.tex_base + 3 * k) * 4];
            std::printf(" %u,%u,%u,%u", word(&o[0]), word(&o[1]), word(&o[2]), word(&o[4]));
        }
        std::printf("\nemitter_meta");                                 // per emitter: the second float4 as words, and word 2 of its grid
        for (uint32_t e = 0; e < s.d.n_emitters; ++e)
            std::printf(" %u,%u,%u,%u,%u", word(&t.emitters[e * 8 + 4]), word(&t.emitters[e * 8 + 5]), word(&t.emitters[e * 8 + 6]), word(&t.emitters[e * 8 + 7]),
                        word(&t.emitter_grid[e * 4 + 2]));
        std::printf("\ncdf");
        for (float v : t.cdf_all) std::printf(" %.9g", v);
        std::printf("\ntypes");
        for (int32_t v : t.emitter_types) std::printf(" e%d", v);
        for (int32_t v : t.bsdf_types) std::printf(" b%d", v);
        std::printf("\n");
        print_vec("pos", t.pos); print_vec("tv", t.tv); print_vec("tn", t.tn); print_vec("tuv", t.tuv); print_vec("mesh_info", t.mesh_info);
        print_vec("bsdfs", t.bsdfs); print_vec("emitters", t.emitters); print_vec("d65", t.d65); print_vec("emitter_grid", t.emitter_grid);
        print_vec("cdf_all", t.cdf_all); print_vec("spectra_pool", t.spectra_pool); print_vec("cie", t.cie); print_vec("texels", t.texels);
        // the tree the tables lead to, with the material classes in its triangle records (tag_classes)
        mskbvh::Built bvh = mskbvh::build(t.pos.data(), s.d.n_faces, t.tri_pad);
        if (!t.all_diffuse) mskscene::tag_classes(bvh, t, &s.d);
        std::printf("classes");
        for (uint32_t f = 0; f < s.d.n_faces; ++f) { const uint32_t w = word(&bvh.tris[(size_t) f * 16 + 3]); std::printf(" %u:%u", w & 0x03ffffffu, w >> MSK_CLASS_SHIFT); }
        std::printf("\n");
        print_vec("bvh_nodes", bvh.nodes); print_vec("bvh_tris", bvh.tris); print_vec("bvh_bounds", bvh.bounds);
    }
    return 0;
}

// ----------------------------------------------------------------------------- placement
static int placement() {
    using namespace mskplan;
    const SceneKnobs knobs = read_scene_knobs();
    // {n_nodes, n_tris, max_depth}: the cbox class; 48 KB of tree met exactly and missed by a node (200 nodes + 379 triangles =
    // 49184 B, one node fewer 49120); 48 KB of tree with a stack of 16 KB (64 KB in all) and of 20 KB; the mesh class; a deep tree
    static const uint32_t trees[7][3] = {{31, 32, 6}, {199, 379, 9}, {200, 379, 9}, {3, 510, 11}, {3, 510, 15}, {40000, 70000, 24}, {3000, 3001, 250}};
    // the wide forms a collapse would give: {8-wide ok, max_depth8, max_depth4, half form, byte form}
    static const int wides[4][5] = {{1, 3, 5, 1, 1}, {0, 0, 7, 1, 1}, {1, 2, 12, 0, 1}, {1, 9, 40, 0, 0}};
    for (const auto &tr : trees)
        for (int leaf_root = 0; leaf_root < 2; ++leaf_root)
            for (const auto &wd : wides) {
                BinaryTree b;
                b.n_nodes = tr[0]; b.n_tris = tr[1]; b.max_depth = (int) tr[2]; b.root_is_leaf = leaf_root != 0;
                std::string asked;
                const TreePlacement p = place_tree(b, knobs, [&](int width) {
                    asked += width == 8 ? "8" : "4";
                    WideTree w;
                    w.ok = width == 4 || wd[0]; w.max_depth = width == 8 ? wd[1] : wd[2]; w.n_nodes = b.n_nodes / 2 + 1;
                    w.has_half = width == 4 && wd[3]; w.has_byte = width == 4 && wd[4];
                    return w;
                });
                std::printf("tree %u %u %d %d %d %d %d %d %d | %d %d %u %u %zu %zu %s\n", b.n_nodes, b.n_tris, b.max_depth, (int) b.root_is_leaf, wd[0], wd[1], wd[2], wd[3], wd[4],
                            p.trace_mode, (int) p.lds_scene, p.stack_entries, p.stack_total, p.trace_lds_bytes, p.binary_stack_bytes, asked.empty() ? "-" : asked.c_str());
            }
    // {n_faces, n_meshes, n_bsdfs, n_textures, n_emitters, cdf_len, n_regular_values}: the cbox; table_f4 2560 / 2561; small_f4 1024 / 1025;
    // nothing at all; many emitters
    static const uint32_t counts[8][7] = {{32, 8, 8, 0, 1, 3, 0}, {396, 10, 10, 1, 1, 3, 4}, {396, 10, 10, 1, 1, 3, 5}, {4000, 90, 118, 2, 1, 3, 8}, {4000, 90, 118, 2, 1, 3, 9},
                                          {0, 0, 0, 0, 0, 1, 0}, {2000, 1000, 1, 0, 999, 2997, 0}, {70000, 3, 3, 1, 2, 8008, 190}};
    for (const auto &c : counts) {
        TableCounts tc;
        tc.n_tris = c[0]; tc.n_meshes = c[1]; tc.n_bsdf_f4 = std::max(1u, c[2]) * MSK_BSDF_F4 + c[3] * 3; tc.n_emitters = c[4]; tc.cdf_len = c[5]; tc.n_spectra = c[6];
        const TablePlacement p = place_tables(tc);
        std::printf("sizes %u %u %u %u %u %u %u | %zu %zu %d %zu %zu\n", c[0], c[1], c[2], c[3], c[4], c[5], c[6], table_bytes(tc), small_bytes(tc), (int) p.lds_tables,
                    p.staged_bytes, p.shade_lds_bytes);
    }
    return 0;
}

int main(int argc, char **argv) {
    if (argc == 2 && !std::strcmp(argv[1], "refusals")) return refusals();
    if (argc == 2 && !std::strcmp(argv[1], "tables")) return tables();
    if (argc == 2 && !std::strcmp(argv[1], "placement")) return placement();
    std::fprintf(stderr, "usage: scene_tables_check refusals|tables|placement\n");
    return 2;
}
