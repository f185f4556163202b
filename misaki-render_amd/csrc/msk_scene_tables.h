// msk_scene_tables.h — what msk_gpu_scene_create* does before it touches the device: every refusal of an msk_scene_desc /
// msk_scene_ext, and the host-side tables the kernels read (per-triangle vertex, normal and uv records; mesh, BSDF, texture,
// spectrum and emitter records; area CDFs; the texel pool with the envmap block; the padding of the boxes; the scene's flags).
// Plain C++17, no HIP: msk_gpu.hip uploads what pack() returns, and tests/native/scene_tables_check.cpp checks every refusal and
// every packed byte on a CPU.  The record layouts are those of msk_kernels.h (DeviceScene); the constants they share: msk_layout.h.
#pragma once
#include "msk_layout.h"
#include "msk_bvh.h"
#include "msk_envmap.h"
#include "../../include/msk_gpu.h"

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "msk_mask_tables.h"
#include "msk_light_tables.h"
#include "msk_plastic_tables.h"

namespace mskscene {

struct HostTables {
    std::vector<float> pos;                 // 9 floats per triangle, scene-global order: what the tree is built from
    std::vector<float> tv, tn, tuv;         // tri_verts (3 float4: p0|mesh p1|- p2|-), tri_normals (3 float4), tri_uvs (2 float4); tn / tuv empty
    bool any_normals = false, any_uvs = false;      // ... unless a mesh has normals / texcoords
    std::vector<int32_t> mesh_info;         // int4 per mesh: bsdf, emitter, has_normals | has_texcoords << 1, first_face
    std::vector<float> bsdfs;               // n_bsdf_f4 float4: MSK_BSDF_F4 per BSDF (at least one), then 3 per texture
    uint32_t n_bsdf_f4 = 0;
    std::vector<float> emitters, d65, emitter_grid, cdf_all;    // 2 float4, 95 floats and 1 float4 per emitter; the area emitters' CDFs
    std::vector<float> spectra_pool, cie;   // the tabulated spectra's values; the CIE 1931 table
    std::vector<float> texels;              // one float4 per bitmap texel, the envmap emitter's block behind them; empty without either
    int env_emitter = -1;                   // index of the environment emitter (`constant` or `envmap`)
    float env_radius = 0.f;                 // ... and the radius of its sphere around the scene
    float tri_pad = 0.f, scene_lo[3] = {INFINITY, INFINITY, INFINITY}, scene_hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    std::vector<int32_t> emitter_types, bsdf_types;      // msk_gpu_point_sample / msk_gpu_conductor_sample check their index against these
    uint32_t n_textures = 0, tex_base = 0;  // msk_gpu_eval_texture: texture k's record sits at float4 tex_base + 3 k of `bsdfs`
    // the scene's flags (mskplan::SceneFacts), final when pack() returns
    bool all_diffuse = true, has_regular = false, has_dielectric = false, has_bitmap = false, has_envmap = false, has_delta = false;
    // a `mask` (msk_mask_tables.h): every BSDF entry then has a mask record at the end of `bsdfs`, from float4 mask_base on;
    // has_mask_image: an opacity is an image, whose values lie behind everything else in `texels`.  Set by pack_masks()
    bool has_mask = false, has_mask_image = false;
    uint32_t mask_base = 0;
    // a `plastic` or a `roughplastic` (MSK_BSDF_PLASTIC, MSK_BSDF_ROUGHPLASTIC, msk_plastic_tables.h): the scene runs the kernels a mask scene runs, and has the mask records whether
    // it holds a mask or not (has_mask says whether it holds one)
    bool has_plastic = false;
};

static inline float h_dot(const float *a, const float *b) { return a[0] * b[0] + (a[1] * b[1] + a[2] * b[2]); }

// the text of a refusal, as msk_gpu.hip's fail_to writes it
inline int refuse(std::string *msg, int code, const char *fmt, ...) {
    char buf[1024];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
    *msg = buf;
    return code;
}

// A HostTables under construction: the descriptor, where a refusal's text goes, and what one table's function leaves for another's.
// The functions run in the order of run(); the order of the checks decides which message a doubly invalid descriptor gets.
struct Packer : HostTables {
    const msk_scene_desc *d;
    const msk_scene_ext *ext;
    const msk_envmap_desc *env;
    const char *pad_scale_text;             // MSK_PAD_SCALE as the environment holds it, or nullptr
    std::string *msg;
    std::vector<float> mesh_area;
    std::vector<std::vector<float>> mesh_cdf;
    mskenv::Tables env_tables;
    uint32_t n_masks;
    const msk_mask_desc *masks;
    std::vector<float> mask_values;         // the mask images' values, in the order of `masks`
    uint32_t n_lights;
    const msk_light_desc *lights;           // what msk_scene_lights holds beyond msk_scene_masks
    bool has_directional = false;           // a sun needs env_radius, with or without an environment emitter

    Packer(const msk_scene_desc *d_, const msk_scene_ext *ext_, const char *pad_scale_text_, std::string *msg_, uint32_t n_masks_ = 0,
           const msk_mask_desc *masks_ = nullptr, uint32_t n_lights_ = 0, const msk_light_desc *lights_ = nullptr)
        : d(d_), ext(ext_), env(ext_ ? ext_->envmap : nullptr), pad_scale_text(pad_scale_text_), msg(msg_), n_masks(n_masks_), masks(masks_),
          n_lights(n_lights_), lights(lights_) {}

    int run() {
        int rc;
        if ((rc = check_header()) || (rc = pack_meshes()) || (rc = check_regular_spectra()) || (rc = pack_textures()) || (rc = pack_bsdfs()) ||
            (rc = pack_masks()) || (rc = pack_emitters()) || (rc = pack_envmap())) return rc;
        if (has_regular) all_diffuse = false;              // tabulated spectra are evaluated by the general shading variant only
        spectra_pool.assign(d->regular_values, d->regular_values + d->n_regular_values);
        if (spectra_pool.empty()) spectra_pool.push_back(0.f);
        if (cdf_all.empty()) cdf_all.push_back(0.f);
        if ((rc = pack_bounds())) return rc;
        for (uint32_t e2 = 0; e2 < d->n_emitters; ++e2) emitter_types.push_back(d->emitters[e2].type);
        for (uint32_t b2 = 0; b2 < d->n_bsdfs; ++b2) bsdf_types.push_back(d->bsdfs[b2].type);
        n_textures = d->n_textures; tex_base = std::max(1u, d->n_bsdfs) * MSK_BSDF_F4;
        cie.assign(d->cie1931_xyz, d->cie1931_xyz + 3 * MSK_CIE_SAMPLES);
        pack_texels();
        pack_env_radius();
        if (has_delta) all_diffuse = false;  // the delta light and the mirror live in instantiations of the general shading variant
        if (has_mask) all_diffuse = false;   // ... and the null lobe
        if (has_plastic) all_diffuse = false;
        return MSK_OK;
    }

    // the mask records, behind the texture records in `bsdfs` (msk_mask_tables.h).  A scene without masks gets none: its tables are what they were.
    // A scene with a plastic and no mask gets records of the constant opacity 1 (msk_plastic_tables.h).
    int pack_masks() {
        if (int rc = pack_mask_records(d, n_masks, masks, bsdfs, n_bsdf_f4, has_mask, has_mask_image, mask_base, mask_values, msg)) return rc;
        if (has_plastic && !has_mask) add_unit_mask_records(d->n_bsdfs, bsdfs, n_bsdf_f4, mask_base);
        return MSK_OK;
    }

    int check_header() {
        if (d->abi_version != MSK_ABI_VERSION)
            return refuse(msg, MSK_ERR_INVALID_ARG, "msk_gpu_scene_create: abi_version %u != %u", d->abi_version, MSK_ABI_VERSION);
        if (d->film.width <= 0 || d->film.height <= 0 || !(d->film.filter_radius > 0.f))
            return refuse(msg, MSK_ERR_INVALID_ARG, "msk_gpu_scene_create: invalid film %dx%d radius %g", d->film.width,
                          d->film.height, d->film.filter_radius);
        {   // Film::set_crop_window (film.cpp:51-63); {0, 0} = the whole film
            const int32_t cx = d->film.crop_offset[0], cy = d->film.crop_offset[1], cw = d->film.crop_size[0], ch = d->film.crop_size[1];
            const bool whole = cw == 0 && ch == 0 && cx == 0 && cy == 0;
            if (!whole && (cx < 0 || cy < 0 || cw <= 0 || ch <= 0 || (int64_t) cx + cw > d->film.width || (int64_t) cy + ch > d->film.height))
                return refuse(msg, MSK_ERR_INVALID_ARG, "Invalid crop window specification! offset (%d, %d) + crop size (%d, %d) vs full size (%d, %d)",
                              cx, cy, cw, ch, d->film.width, d->film.height);
        }
        if (!d->cie1931_xyz || !d->d65) return refuse(msg, MSK_ERR_INVALID_ARG, "msk_gpu_scene_create: spectral tables missing");
        if ((d->n_faces && (!d->vertices || !d->faces)) || (d->n_meshes && !d->meshes))
            return refuse(msg, MSK_ERR_INVALID_ARG, "msk_gpu_scene_create: geometry arrays missing");
        if ((d->n_bsdfs && !d->bsdfs) || (d->n_emitters && !d->emitters))
            return refuse(msg, MSK_ERR_INVALID_ARG, "msk_gpu_scene_create: bsdf / emitter arrays missing");
        // leaf references pack first_tri << 5 | count into 31 bits (msk_bvh.h) and bit 31 of a hit's prim word is the shadow flag
        if (d->n_faces >= (1u << 26))
            return refuse(msg, MSK_ERR_UNSUPPORTED, "msk_gpu_scene_create: %u triangles, this back end addresses fewer than 2^26", d->n_faces);
        return MSK_OK;
    }

    // per-triangle data, mesh records, the meshes' areas and area CDFs (operand shapes are checked here, on the host, before any
    // kernel can index with them)
    int pack_meshes() {
        pos.assign((size_t) d->n_faces * 9, 0.f);
        tv.assign((size_t) d->n_faces * 12, 0.f);
        mesh_info.assign((size_t) std::max(1u, d->n_meshes) * 4, 0);
        for (uint32_t m = 0; m < d->n_meshes; ++m) {
            const msk_mesh_desc &md = d->meshes[m];
            if ((uint64_t) md.first_vertex + md.vertex_count > d->n_vertices || (uint64_t) md.first_face + md.face_count > d->n_faces)
                return refuse(msg, MSK_ERR_INVALID_ARG, "mesh %u: vertex/face range exceeds the arrays", m);
            if (md.bsdf_id < 0 || (uint32_t) md.bsdf_id >= d->n_bsdfs)
                return refuse(msg, MSK_ERR_INVALID_ARG, "mesh %u: bsdf_id %d out of range", m, md.bsdf_id);
            if (md.emitter_id >= (int32_t) d->n_emitters || md.emitter_id < -1)
                return refuse(msg, MSK_ERR_INVALID_ARG, "mesh %u: emitter_id %d out of range", m, md.emitter_id);
            // one mesh per area emitter, named from both sides (Shape::m_emitter / Emitter::m_shape, shape.cpp:27-37): a second
            // mesh pointing at the same emitter would be lit with the first one's area pdf and CDF
            if (md.emitter_id >= 0 && (!d->emitters || d->emitters[md.emitter_id].mesh_id != (int32_t) m))
                return refuse(msg, MSK_ERR_INVALID_ARG, "mesh %u: emitter %d does not point back at it", m, md.emitter_id);
            any_normals |= md.has_normals != 0; any_uvs |= md.has_texcoords != 0;
        }
        if (any_normals) tn.assign((size_t) d->n_faces * 12, 0.f);
        if (any_uvs) tuv.assign((size_t) d->n_faces * 8, 0.f);
        std::vector<uint8_t> covered(d->n_faces, 0);
        mesh_area.assign(d->n_meshes, 0.f);
        mesh_cdf.assign(d->n_meshes, std::vector<float>());
        for (uint32_t m = 0; m < d->n_meshes; ++m) {
            const msk_mesh_desc &md = d->meshes[m];
            mesh_info[m * 4 + 0] = md.bsdf_id; mesh_info[m * 4 + 1] = md.emitter_id;
            mesh_info[m * 4 + 2] = (md.has_normals ? 1 : 0) | (md.has_texcoords ? 2 : 0);
            mesh_info[m * 4 + 3] = (int32_t) md.first_face;
            // mesh.cpp:39-48 area_distr_build + core/distribution.h:88-96 (fp32, started from 0)
            float surface_area = 0.f, run = 0.f;
            std::vector<float> &cdf = mesh_cdf[m];
            cdf.push_back(0.f);
            for (uint32_t f = 0; f < md.face_count; ++f) {
                const uint32_t g = md.first_face + f;
                if (covered[g]) return refuse(msg, MSK_ERR_INVALID_ARG, "face %u belongs to two meshes", g);
                covered[g] = 1;
                const uint32_t *fi = d->faces + (size_t) g * 3;
                const float *v[3];
                for (int k = 0; k < 3; ++k) {
                    if (fi[k] >= md.vertex_count) return refuse(msg, MSK_ERR_INVALID_ARG, "mesh %u face %u: vertex index %u out of range", m, f, fi[k]);
                    v[k] = d->vertices + (size_t) (md.first_vertex + fi[k]) * 8;
                    if (!(std::isfinite(v[k][0]) && std::isfinite(v[k][1]) && std::isfinite(v[k][2])))
                        return refuse(msg, MSK_ERR_INVALID_ARG, "mesh %u vertex %u: non-finite position", m, fi[k]);
                    for (int c = 0; c < 3; ++c) { pos[(size_t) g * 9 + k * 3 + c] = v[k][c]; tv[(size_t) g * 12 + k * 4 + c] = v[k][c]; }
                    if (any_normals) for (int c = 0; c < 3; ++c) tn[(size_t) g * 12 + k * 4 + c] = v[k][3 + c];
                }
                uint32_t mb = m; std::memcpy(&tv[(size_t) g * 12 + 3], &mb, 4);
                if (any_uvs) {
                    float *u = &tuv[(size_t) g * 8];
                    u[0] = v[0][6]; u[1] = v[0][7]; u[2] = v[1][6]; u[3] = v[1][7]; u[4] = v[2][6]; u[5] = v[2][7];
                }
                // mesh.h:54-61 face_area = 0.5 * |(p1-p0) x (p2-p0)|
                const float a[3] = {v[1][0] - v[0][0], v[1][1] - v[0][1], v[1][2] - v[0][2]};
                const float b[3] = {v[2][0] - v[0][0], v[2][1] - v[0][1], v[2][2] - v[0][2]};
                const float cr[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
                const float area = 0.5f * std::sqrt(h_dot(cr, cr));
                surface_area += area;
                run = (f == 0) ? area : run + area;
                cdf.push_back(run);
            }
            if (md.face_count) { const float inv_sum = 1.f / cdf.back(); for (auto &c : cdf) c *= inv_sum; }
            mesh_area[m] = surface_area;
        }
        for (uint32_t g = 0; g < d->n_faces; ++g)
            if (!covered[g]) return refuse(msg, MSK_ERR_INVALID_ARG, "face %u belongs to no mesh", g);
        return MSK_OK;
    }

    // tabulated (`regular`) spectra, ABI v7 (spectra/regular.cpp:27-70): validated here, before any kernel indexes with them
    int check_regular_spectra() {
        if ((d->n_regular_spectra && !d->regular_spectra) || (d->n_regular_values && !d->regular_values))
            return refuse(msg, MSK_ERR_INVALID_ARG, "msk_gpu_scene_create: regular spectrum arrays missing");
        if (d->n_regular_values >= (1u << 24))
            return refuse(msg, MSK_ERR_UNSUPPORTED, "msk_gpu_scene_create: %u tabulated spectrum values, a spectrum record addresses fewer than 2^24", d->n_regular_values);
        for (uint32_t k = 0; k < d->n_regular_spectra; ++k) {
            const msk_regular_spectrum_desc &r = d->regular_spectra[k];
            if (r.size < 2) return refuse(msg, MSK_ERR_INVALID_ARG, "regular spectrum %u: ContinuousDistribution: needs at least two entries!", k);     // regular.cpp:30-31
            if (r.size > MSK_REGULAR_MAX) return refuse(msg, MSK_ERR_UNSUPPORTED, "regular spectrum %u: %u values, this back end takes at most %d", k, r.size, MSK_REGULAR_MAX);
            if (!(r.lambda_min < r.lambda_max) || !std::isfinite(r.lambda_min) || !std::isfinite(r.lambda_max))
                return refuse(msg, MSK_ERR_INVALID_ARG, "regular spectrum %u: ContinuousDistribution: invalid range!", k);                                // regular.cpp:33-34
            if ((uint64_t) r.first_value + r.size > d->n_regular_values)
                return refuse(msg, MSK_ERR_INVALID_ARG, "regular spectrum %u: values [%u, %u) exceed the %u in regular_values", k, r.first_value, r.first_value + r.size, d->n_regular_values);
            bool mass = false;
            for (uint32_t i = 0; i < r.size; ++i) {
                const float v = d->regular_values[r.first_value + i];
                if (!(v >= 0.f) || !std::isfinite(v)) return refuse(msg, MSK_ERR_INVALID_ARG, "regular spectrum %u: ContinuousDistribution: entries must be non-negative!", k);   // regular.cpp:59-60
                mass |= v > 0.f;
            }
            if (!mass) return refuse(msg, MSK_ERR_INVALID_ARG, "regular spectrum %u: ContinuousDistribution: no probability mass found!", k);            // regular.cpp:73-74
        }
        return MSK_OK;
    }
    // 1 / interval as RegularSpectrum keeps it: the interval in double, its reciprocal rounded to float (regular.cpp:42-43,66-70)
    static float inv_interval(const msk_regular_spectrum_desc &r) { return (float) (1.0 / (((double) r.lambda_max - (double) r.lambda_min) / (double) (r.size - 1))); }
    // device form of an msk_spectrum_desc: {c0, c1, c2, scale} or {lambda_min, inv_interval, first | last << 24, -1} (msk_kernels.h: spectrum_eval)
    int spectrum_record(const msk_spectrum_desc &sp, float *o, const char *what, uint32_t b) {
        if (sp.regular) {
            if (sp.regular > d->n_regular_spectra) return refuse(msg, MSK_ERR_INVALID_ARG, "bsdf %u: %s names regular spectrum %u of %u", b, what, sp.regular, d->n_regular_spectra);
            const msk_regular_spectrum_desc &r = d->regular_spectra[sp.regular - 1];
            const uint32_t w = r.first_value | ((r.size - 2u) << 24);
            o[0] = r.lambda_min; o[1] = inv_interval(r); std::memcpy(&o[2], &w, 4); o[3] = -1.f;
            has_regular = true;
            return MSK_OK;
        }
        if (!(sp.scale >= 0.f)) return refuse(msg, MSK_ERR_INVALID_ARG, "bsdf %u: the scale of %s must not be negative", b, what);
        o[0] = sp.coeff[0]; o[1] = sp.coeff[1]; o[2] = sp.coeff[2]; o[3] = sp.scale;
        return MSK_OK;
    }

    // the texture records, behind the BSDF records in `bsdfs`
    int pack_textures() {
        if (d->n_textures && !d->textures) return refuse(msg, MSK_ERR_INVALID_ARG, "msk_gpu_scene_create: texture array missing");
        n_bsdf_f4 = std::max(1u, d->n_bsdfs) * MSK_BSDF_F4 + d->n_textures * 3;
        bsdfs.assign((size_t) n_bsdf_f4 * 4, 0.f);
        for (uint32_t t = 0; t < d->n_textures; ++t) {
            const msk_texture_desc &td = d->textures[t];
            if (td.type != MSK_TEXTURE_CHECKERBOARD && td.type != MSK_TEXTURE_BITMAP && td.type != MSK_TEXTURE_BITMAP_NEAREST)
                return refuse(msg, MSK_ERR_UNSUPPORTED, "texture %u: type %d is not supported by this back end (checkerboard, bitmap)", t, td.type);
            float *o = &bsdfs[((size_t) std::max(1u, d->n_bsdfs) * MSK_BSDF_F4 + (size_t) t * 3) * 4];
            if (td.type != MSK_TEXTURE_CHECKERBOARD) {
                if (td.width < 1 || td.height < 1)
                    return refuse(msg, MSK_ERR_INVALID_ARG, "texture %u: a bitmap of %u x %u texels (width and height must be at least 1)", t, td.width, td.height);
                if ((uint64_t) td.first_texel + (uint64_t) td.width * td.height > d->n_texels)
                    return refuse(msg, MSK_ERR_INVALID_ARG, "texture %u: texels %u + %u x %u reach past the scene's n_texels %u", t, td.first_texel, td.width,
                                  td.height, d->n_texels);
                if (!d->texels) return refuse(msg, MSK_ERR_INVALID_ARG, "texture %u: a bitmap, but the scene's texels array is missing", t);
                const size_t n = (size_t) td.width * td.height * 3;
                for (size_t k = 0; k < n; ++k)
                    if (std::isnan(d->texels[(size_t) td.first_texel * 3 + k]))
                        return refuse(msg, MSK_ERR_INVALID_ARG, "texture %u: texel %zu holds a NaN coefficient", t, k / 3);
                const uint32_t w[3] = {td.first_texel, td.width, td.height}, ty = (uint32_t) td.type;
                std::memcpy(&o[0], w, 12); o[3] = td.to_uv[2];
                std::memcpy(&o[4], &ty, 4); o[5] = 0.f; o[6] = 0.f; o[7] = td.to_uv[5];
                o[8] = td.to_uv[0]; o[9] = td.to_uv[1]; o[10] = td.to_uv[3]; o[11] = td.to_uv[4];
                has_bitmap = true;
                continue;
            }
            o[0] = td.color0[0]; o[1] = td.color0[1]; o[2] = td.color0[2]; o[3] = td.to_uv[2];
            o[4] = td.color1[0]; o[5] = td.color1[1]; o[6] = td.color1[2]; o[7] = td.to_uv[5];
            o[8] = td.to_uv[0]; o[9] = td.to_uv[1]; o[10] = td.to_uv[3]; o[11] = td.to_uv[4];
        }
        return MSK_OK;
    }

    int pack_bsdfs() {
        int rc_spec = MSK_OK;
        for (uint32_t b = 0; b < d->n_bsdfs; ++b) {
            const msk_bsdf_desc &bd = d->bsdfs[b];
            if (bd.type != MSK_BSDF_DIFFUSE && bd.type != MSK_BSDF_ROUGHCONDUCTOR && bd.type != MSK_BSDF_ROUGHDIELECTRIC && bd.type != MSK_BSDF_DIELECTRIC &&
                bd.type != MSK_BSDF_CONDUCTOR && bd.type != MSK_BSDF_PLASTIC && bd.type != MSK_BSDF_ROUGHPLASTIC)
                return refuse(msg, MSK_ERR_UNSUPPORTED,
                              "bsdf %u: type %d is not supported by this back end (diffuse, roughconductor, roughdielectric, dielectric, conductor)", b, bd.type);
            if (bd.back_bsdf >= (int32_t) d->n_bsdfs || bd.back_bsdf < -1)
                return refuse(msg, MSK_ERR_INVALID_ARG, "bsdf %u: back_bsdf %d out of range", b, bd.back_bsdf);
            const bool rough_coat = bd.type == MSK_BSDF_ROUGHPLASTIC, plastic = bd.type == MSK_BSDF_PLASTIC || rough_coat;
            const bool has_rho = bd.type == MSK_BSDF_DIFFUSE || plastic;      // a plastic's base is the diffuse BSDF's reflectance
            if (!has_rho && !(bd.alpha_u >= 0.f && bd.alpha_v >= 0.f))
                return refuse(msg, MSK_ERR_INVALID_ARG, "bsdf %u: negative roughness", b);
            if ((bd.type == MSK_BSDF_ROUGHDIELECTRIC || bd.type == MSK_BSDF_DIELECTRIC) && !(bd.ior_eta > 0.f && bd.ior_inv_eta > 0.f))
                return refuse(msg, MSK_ERR_INVALID_ARG, "bsdf %u: the relative index of refraction must be positive", b);
            if (bd.type == MSK_BSDF_DIELECTRIC && bd.back_bsdf >= 0)                                         // twosided.cpp:33-35
                return refuse(msg, MSK_ERR_INVALID_ARG, "bsdf %u: Only materials without a transmission component can be nested!", b);
            if (bd.type == MSK_BSDF_DIELECTRIC) has_dielectric = true;
            // Why this check exists: until the smooth conductor, type 4 was the first unassigned BSDF type, and tests/test_smooth_dielectric.py
            // (an existing file, which a feature does not edit) creates a `dielectric` descriptor, overwrites its type with 4 and expects
            // the refusal "type 4 is not supported".  A conductor has no relative index of refraction: both flatteners write 1 / 1 and a
            // zero-filled descriptor carries 0 / 0.  A type-4 descriptor with any other index is a descriptor of another kind relabelled,
            // and it keeps being refused with those words instead of being rendered as a mirror.
            if (bd.type == MSK_BSDF_CONDUCTOR && !((bd.ior_eta == 1.f && bd.ior_inv_eta == 1.f) || (bd.ior_eta == 0.f && bd.ior_inv_eta == 0.f)))
                return refuse(msg, MSK_ERR_INVALID_ARG, "bsdf %u: type %d is not supported for a descriptor with a relative index of refraction (ior_eta %g, ior_inv_eta %g): "
                              "a conductor has none (1 / 1, or 0 / 0 = unset); its eta and k are spectra", b, bd.type, (double) bd.ior_eta, (double) bd.ior_inv_eta);
            if (bd.type == MSK_BSDF_CONDUCTOR) has_delta = true;
            if (plastic) { if (int rc = rough_coat ? check_roughplastic(bd, b, msg) : check_plastic(bd, b, msg)) return rc; has_plastic = true; }
            if (bd.reflectance_texture > d->n_textures)
                return refuse(msg, MSK_ERR_INVALID_ARG, "bsdf %u: reflectance_texture %u out of range", b, bd.reflectance_texture);
            if (has_rho && !bd.reflectance_regular && !(bd.reflectance_scale >= 0.f && bd.reflectance_scale < INFINITY))
                return refuse(msg, MSK_ERR_INVALID_ARG, "bsdf %u: reflectance_scale must be finite and non-negative (1 for an srgb reflectance)", b);
            if (bd.reflectance_texture && !has_rho)
                return refuse(msg, MSK_ERR_UNSUPPORTED, "bsdf %u: only the diffuse reflectance can be textured", b);
            if (bd.reflectance_regular && (!has_rho || bd.reflectance_texture))
                return refuse(msg, MSK_ERR_INVALID_ARG, "bsdf %u: reflectance_regular names the reflectance of an untextured diffuse BSDF", b);
            if (bd.type != MSK_BSDF_DIFFUSE || bd.back_bsdf >= 0 || bd.reflectance_texture || bd.reflectance_regular) all_diffuse = false;
            // the device record, MSK_BSDF_F4 float4 (msk_kernels.h: BsdfRec): {type, back, r0, r1} {r2, au, av, sample_visible} eta k
            // spec trans {ior_eta, ior_inv_eta, float4 offset of the texture record, reflectance_scale}
            float *o = &bsdfs[(size_t) b * 4 * MSK_BSDF_F4];
            std::memcpy(&o[0], &bd.type, 4); std::memcpy(&o[1], &bd.back_bsdf, 4);
            msk_spectrum_desc refl;
            refl.coeff[0] = bd.reflectance[0]; refl.coeff[1] = bd.reflectance[1]; refl.coeff[2] = bd.reflectance[2];
            refl.scale = has_rho ? bd.reflectance_scale : 0.f; refl.regular = bd.reflectance_regular;
            float r4[4] = {};
            if ((rc_spec = spectrum_record(refl, r4, "reflectance", b))) return rc_spec;
            o[2] = r4[0]; o[3] = r4[1]; o[4] = r4[2];
            o[5] = bd.alpha_u; o[6] = bd.alpha_v; std::memcpy(&o[7], &bd.sample_visible, 4);
            if ((rc_spec = spectrum_record(bd.eta, &o[8], "eta", b)) || (rc_spec = spectrum_record(bd.k, &o[12], "k", b)) ||
                (rc_spec = spectrum_record(bd.specular_reflectance, &o[16], "specular_reflectance", b)) ||
                (rc_spec = spectrum_record(bd.specular_transmittance, &o[20], "specular_transmittance", b))) return rc_spec;
            o[24] = bd.ior_eta; o[25] = bd.ior_inv_eta;
            const uint32_t tex_off = bd.reflectance_texture ? std::max(1u, d->n_bsdfs) * MSK_BSDF_F4 + (bd.reflectance_texture - 1) * 3 : 0u;
            std::memcpy(&o[26], &tex_off, 4);
            o[27] = r4[3];                                             // reflectance_scale, or -1 for a tabulated reflectance
            if (plastic) {                                             // {fdr_int, ssw} where the rough types keep alpha_u, alpha_v (the roughplastic, which
                plastic_constants(d, bd, &o[plastic_constants_word(bd.type)]);      // keeps its alpha there: in two words of `trans`); `nonlinear` as 0 / 1
                const int32_t nonlinear = bd.sample_visible != 0 ? 1 : 0;
                std::memcpy(&o[7], &nonlinear, 4);
            }
        }
        return MSK_OK;
    }

    // emitter records, their D65 tables and grids, the area emitters' CDFs; then the msk_point_desc and msk_light_desc lists themselves
    int pack_emitters() {
        if (int rc = check_light_list(n_lights, lights, msg)) return rc;
        emitters.assign((size_t) std::max(1u, d->n_emitters) * 8, 0.f); d65.assign((size_t) std::max(1u, d->n_emitters) * 95, 0.f);
        emitter_grid.assign((size_t) std::max(1u, d->n_emitters) * 4, 0.f);
        for (uint32_t e = 0; e < d->n_emitters; ++e) {
            const msk_emitter_desc &ed = d->emitters[e];
            float *o = &emitters[e * 8];
            o[0] = ed.radiance[0]; o[1] = ed.radiance[1]; o[2] = ed.radiance[2];
            if (ed.type == MSK_EMITTER_CONSTANT || ed.type == MSK_EMITTER_ENVMAP) {
                if (ed.type == MSK_EMITTER_ENVMAP) {
                    if (!env) return refuse(msg, MSK_ERR_INVALID_ARG, "emitter %u: an envmap emitter needs its image (msk_gpu_scene_create_env with an msk_envmap_desc)", e);
                    if (ed.radiance_regular) return refuse(msg, MSK_ERR_INVALID_ARG, "emitter %u: an envmap emitter has no tabulated radiance (radiance_regular must be 0)", e);
                    if (!(ed.d65_scale >= 0.f) || !std::isfinite(ed.d65_scale)) return refuse(msg, MSK_ERR_INVALID_ARG, "emitter %u: envmap: the scale must be finite and non-negative", e);
                    has_envmap = true;
                    o[0] = 0.f; o[1] = 0.f; o[2] = INFINITY;      // the emitter's own factor is its table alone: S = 1
                }
                if (env_emitter >= 0) return refuse(msg, MSK_ERR_INVALID_ARG, "Can only have one environment light");   // scene.cpp:38-39
                if (ed.mesh_id != -1) return refuse(msg, MSK_ERR_INVALID_ARG, "emitter %u: an environment emitter has no mesh (mesh_id must be -1)", e);
                env_emitter = (int) e;
                o[3] = 0.f;
                // (an envmap: word 1 = the float4 offset of its block in the texel pool, behind the bitmaps' texels — msk_kernels.h, EnvView)
                // word 2 = 1 for an image, 0 for the `constant` sky: what the kernels that serve both read (env_is_image)
                const uint32_t meta[4] = {0xffffffffu, ed.type == MSK_EMITTER_ENVMAP ? d->n_texels : 0u, ed.type == MSK_EMITTER_ENVMAP ? 1u : 0u, 0u};
                std::memcpy(&o[4], meta, 16);
            } else if (ed.type == MSK_EMITTER_AREA) {
                if (ed.mesh_id < 0 || (uint32_t) ed.mesh_id >= d->n_meshes || d->meshes[ed.mesh_id].emitter_id != (int32_t) e)
                    return refuse(msg, MSK_ERR_INVALID_ARG, "emitter %u: mesh_id %d does not point back at it", e, ed.mesh_id);
                const msk_mesh_desc &md = d->meshes[ed.mesh_id];
                if (md.face_count == 0) return refuse(msg, MSK_ERR_INVALID_ARG, "emitter %u: its mesh has no faces", e);
                o[3] = 1.f / mesh_area[ed.mesh_id];                               // mesh.cpp:129 ps.pdf
                uint32_t meta[4] = {(uint32_t) ed.mesh_id, md.first_face, md.face_count, (uint32_t) cdf_all.size()};
                std::memcpy(&o[4], meta, 16);
                cdf_all.insert(cdf_all.end(), mesh_cdf[ed.mesh_id].begin(), mesh_cdf[ed.mesh_id].end());
            } else if (ed.type == MSK_EMITTER_POINT) {
                // point.cpp: the intensity in the radiance's place; the position behind a type marker (msk_layout.h: MSK_EMITTER_MARK_POINT)
                if (ed.mesh_id != -1) return refuse(msg, MSK_ERR_INVALID_ARG, "emitter %u: a point emitter has no mesh (mesh_id must be -1)", e);
                const msk_point_desc *pd = nullptr;
                for (uint32_t k = 0; ext && k < ext->n_points; ++k)
                    if (ext->points && ext->points[k].emitter == e) {
                        if (pd) return refuse(msg, MSK_ERR_INVALID_ARG, "emitter %u: a point emitter with two positions (msk_point_desc %u is its second)", e, k);
                        pd = &ext->points[k];
                    }
                if (!pd) return refuse(msg, MSK_ERR_INVALID_ARG, "emitter %u: a point emitter needs its position (msk_gpu_scene_create_ext with an msk_point_desc)", e);
                if (!std::isfinite(pd->position[0]) || !std::isfinite(pd->position[1]) || !std::isfinite(pd->position[2]))
                    return refuse(msg, MSK_ERR_INVALID_ARG, "emitter %u: a point emitter's position must be finite", e);
                has_delta = true;
                o[3] = 0.f;
                const uint32_t mark = MSK_EMITTER_MARK_POINT;
                std::memcpy(&o[4], &mark, 4); std::memcpy(&o[5], pd->position, 12);
            } else if (ed.type == MSK_EMITTER_SPOT || ed.type == MSK_EMITTER_DIRECTIONAL) {
                if (int rc = pack_light_record(e, ed, n_lights, lights, o, cdf_all, has_delta, has_directional, msg)) return rc;      // msk_light_tables.h
            } else {
                return refuse(msg, MSK_ERR_UNSUPPORTED, "emitter %u: type %d is not supported (area, constant, envmap, point)", e, ed.type);
            }
            float *gr = &emitter_grid[(size_t) e * 4];
            if (ed.radiance_regular) {          // a `regular` radiance: its own table on its own grid, no sigmoid factor (area.cpp:51-54, regular.cpp:148)
                if (ed.radiance_regular > d->n_regular_spectra) return refuse(msg, MSK_ERR_INVALID_ARG, "emitter %u: radiance names regular spectrum %u of %u", e, ed.radiance_regular, d->n_regular_spectra);
                const msk_regular_spectrum_desc &r = d->regular_spectra[ed.radiance_regular - 1];
                for (uint32_t i = 0; i < r.size; ++i) d65[e * 95 + i] = d->regular_values[r.first_value + i];
                const uint32_t last = r.size - 2u;
                gr[0] = r.lambda_min; gr[1] = inv_interval(r); std::memcpy(&gr[2], &last, 4); gr[3] = 1.f;
                o[0] = o[1] = 0.f; o[2] = INFINITY;
                has_regular = true;
            } else {
                for (int i = 0; i < 95; ++i) d65[e * 95 + i] = d->d65[i] * ed.d65_scale;   // d65.cpp:41-42
                const uint32_t last = 93u;
                gr[0] = 360.f; gr[1] = (float) (1.0 / ((830.0 - 360.0) / 94.0)); std::memcpy(&gr[2], &last, 4); gr[3] = 0.f;
            }
        }
        for (uint32_t k = 0; ext && k < ext->n_points; ++k) {
            if (!ext->points) return refuse(msg, MSK_ERR_INVALID_ARG, "msk_scene_ext: n_points %u without points", ext->n_points);
            const uint32_t pe = ext->points[k].emitter;
            if (pe >= d->n_emitters) return refuse(msg, MSK_ERR_INVALID_ARG, "msk_point_desc %u: emitter %u out of range (the scene has %u)", k, pe, d->n_emitters);
            if (d->emitters[pe].type != MSK_EMITTER_POINT)
                return refuse(msg, MSK_ERR_INVALID_ARG, "msk_point_desc %u: emitter %u is of type %d, not a point emitter (type %d)", k, pe, d->emitters[pe].type, MSK_EMITTER_POINT);
        }
        if (int rc = check_light_emitters(d, n_lights, lights, msg)) return rc;
        return MSK_OK;
    }

    // the image of the envmap emitter (msk_gpu.h: msk_envmap_desc; msk_envmap.h): validated here, before any kernel indexes with it
    int pack_envmap() {
        if (env && !has_envmap) return refuse(msg, MSK_ERR_INVALID_ARG, "envmap: an image was given, but the scene has no envmap emitter (type %d)", MSK_EMITTER_ENVMAP);
        if (has_envmap) {
            if (env->width < 1 || env->height < 1) return refuse(msg, MSK_ERR_INVALID_ARG, "envmap: an image of %u x %u texels (width and height must be at least 1)", env->width, env->height);
            if ((uint64_t) env->width * env->height >= (1ull << 28)) return refuse(msg, MSK_ERR_UNSUPPORTED, "envmap: %u x %u texels, this back end takes fewer than 2^28", env->width, env->height);
            if (!env->texels || !env->weights) return refuse(msg, MSK_ERR_INVALID_ARG, "envmap: texels / weights array missing");
            const size_t n = (size_t) env->width * env->height;
            for (size_t k = 0; k < n; ++k) {
                const float *t = env->texels + k * 4;
                if (!std::isfinite(t[3]) || t[3] < 0.f) return refuse(msg, MSK_ERR_INVALID_ARG, "envmap: texel %zu: the factor w must be finite and non-negative", k);
                if (std::isnan(t[0]) || std::isnan(t[1]) || std::isnan(t[2])) return refuse(msg, MSK_ERR_INVALID_ARG, "envmap: texel %zu holds a NaN coefficient", k);
            }
            if (const char *m = mskenv::check_weights(env->weights, env->width, env->height)) return refuse(msg, MSK_ERR_INVALID_ARG, "%s", m);
            if (!mskenv::is_rotation(env->to_world)) return refuse(msg, MSK_ERR_INVALID_ARG, "envmap: to_world must be a rotation");
            if ((uint64_t) d->n_texels + 3u + n + ((uint64_t) env->height + 4u) / 4u + ((uint64_t) env->height * (env->width + 1u) + 3u) / 4u >= (1ull << 31))
                return refuse(msg, MSK_ERR_UNSUPPORTED, "envmap: %u x %u texels do not fit the texel pool's 32-bit offsets", env->width, env->height);
            env_tables = mskenv::build_tables(env->weights, env->width, env->height);
        }
        return MSK_OK;
    }

    // oracle D10: the triangle-bounds predicate's padding, computed exactly as the oracle does (0.5e-5 of the scene's scale =
    // max(diagonal, largest coordinate magnitude)); node boxes are padded by twice that
    int pack_bounds() {
        float *lo = scene_lo, *hi = scene_hi;
        for (uint32_t t = 0; t < d->n_faces; ++t)
            for (int v = 0; v < 3; ++v)
                for (int k = 0; k < 3; ++k) { const float q = pos[(size_t) t * 9 + v * 3 + k]; lo[k] = std::min(lo[k], q); hi[k] = std::max(hi[k], q); }
        const float ex = hi[0] - lo[0], ey = hi[1] - lo[1], ez = hi[2] - lo[2];
        const float diag = d->n_faces ? std::sqrt(ex * ex + (ey * ey + ez * ez)) : 1.f;
        float amax = 0.f;
        if (d->n_faces) amax = std::max(std::max(std::max(std::fabs(lo[0]), std::fabs(hi[0])), std::max(std::fabs(lo[1]), std::fabs(hi[1]))), std::max(std::fabs(lo[2]), std::fabs(hi[2])));
        // (MSK_PAD_SCALE, read by the oracle too: the margin tests shrink the padding on both sides to show how far the rule is from
        // failing — tree and brute force agree down to 1e-7 of the scale and part at 1e-8, tests/test_padding_margin.py.  A value that
        // is not a number in [1e-7, 1e-3] is refused: zero, garbage or a stray setting would silently remove the padding on both
        // sides of the parity tests at once.)
        float pad_scale = 1e-5f;
        if (const char *ps = pad_scale_text) {
            char *end = nullptr;
            const double v = strtod(ps, &end);
            if (end == ps || *end != '\0' || !std::isfinite(v) || v < 1e-7 || v > 1e-3)
                return refuse(msg, MSK_ERR_INVALID_ARG, "MSK_PAD_SCALE=\"%s\": the padding of the boxes must be a number in [1e-7, 1e-3] of the scene's scale "
                              "(default 1e-5; the slab arithmetic needs a few 1e-7)", ps);
            pad_scale = (float) v;
        }
        tri_pad = (0.5f * pad_scale) * std::max(diag, amax);
        return MSK_OK;
    }

    // one float4 per texel: a lookup is one 16-byte load per texel
    void pack_texels() {
        if (!(has_bitmap || has_envmap || has_mask_image)) return;
        std::vector<float> &tx4 = texels;
        tx4.assign((size_t) d->n_texels * 4, 0.f);
        if (d->texels) for (size_t k = 0; k < d->n_texels; ++k) { tx4[k * 4] = d->texels[k * 3]; tx4[k * 4 + 1] = d->texels[k * 3 + 1]; tx4[k * 4 + 2] = d->texels[k * 3 + 2]; }
        if (has_envmap) {                // the envmap emitter's block behind them (msk_kernels.h, EnvView): header, texels, marginal, rows
            const size_t n = (size_t) env->width * env->height;
            float head[12] = {};
            std::memcpy(&head[0], &env->width, 4); std::memcpy(&head[1], &env->height, 4);
            std::memcpy(&head[2], env->to_world, 36);
            tx4.insert(tx4.end(), head, head + 12);
            tx4.insert(tx4.end(), env->texels, env->texels + n * 4);
            tx4.insert(tx4.end(), env_tables.marg.begin(), env_tables.marg.end());
            tx4.resize((tx4.size() + 3) & ~(size_t) 3, 0.f);
            tx4.insert(tx4.end(), env_tables.cond.begin(), env_tables.cond.end());
            tx4.resize((tx4.size() + 3) & ~(size_t) 3, 0.f);
        }
        if (has_mask_image) place_mask_values(d->n_bsdfs, mask_base, bsdfs, mask_values, tx4);      // the mask images' values behind them (msk_mask_tables.h)
    }

    // constant.cpp:21-28 set_scene: the sphere around Scene::bbox() (bbox.h:105-112), in fp32 exactly as the oracle does.
    // A directional emitter's shadow ray has the same length as an environment emitter's: its scene gets the radius too
    void pack_env_radius() {
        if (env_emitter < 0 && !has_directional) return;
        float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
        for (uint32_t v = 0; v < d->n_vertices; ++v)
            for (int k = 0; k < 3; ++k) { const float q = d->vertices[(size_t) v * 8 + k]; lo[k] = std::min(lo[k], q); hi[k] = std::max(hi[k], q); }
        float r[3];
        for (int k = 0; k < 3; ++k) { const float c = (lo[k] + hi[k]) * .5f; r[k] = c - hi[k]; }
        const float radius = std::sqrt(r[0] * r[0] + (r[1] * r[1] + r[2] * r[2]));
        env_radius = std::max(MSK_RAY_EPS_F, radius * (1.f + MSK_RAY_EPS_F));
        all_diffuse = false;             // the environment terms live in the general shading variant
    }
};

// Fills *out from the descriptor; pad_scale_text = MSK_PAD_SCALE as the environment holds it (mskplan::SceneKnobs), or nullptr.
// MSK_OK, or the code of the first refusal with its text in *msg (*out is then untouched).
// n_masks / masks: what msk_scene_masks holds beyond msk_scene_ext (none: the tables are those of the scene without the argument).
// n_lights / lights: what msk_scene_lights holds beyond msk_scene_masks, likewise.
inline int pack(const msk_scene_desc *d, const msk_scene_ext *ext, const char *pad_scale_text, HostTables *out, std::string *msg, uint32_t n_masks = 0,
                const msk_mask_desc *masks = nullptr, uint32_t n_lights = 0, const msk_light_desc *lights = nullptr) {
    Packer p(d, ext, pad_scale_text, msg, n_masks, masks, n_lights, lights);
    const int rc = p.run();
    if (rc == MSK_OK) *out = std::move(static_cast<HostTables &>(p));
    return rc;
}

// material class of every triangle into its leaf record's prim word (MSK_CLASS_SHIFT): the traversal hands it to the
// shading kernel with the hit, which sorts its paths by it
inline void tag_classes(mskbvh::Built &bvh, const HostTables &t, const msk_scene_desc *d) {
    for (size_t k = 0; k < d->n_faces; ++k) {
        uint32_t w, mesh;
        std::memcpy(&w, &bvh.tris[k * 16 + 3], 4);
        std::memcpy(&mesh, &t.tv[(size_t) w * 12 + 3], 4);
        const int32_t b = t.mesh_info[(size_t) mesh * 4];
        const uint32_t cls = (b >= 0 && (uint32_t) b < d->n_bsdfs) ? (uint32_t) d->bsdfs[b].type : 0u;      // MSK_BSDF_* = 0, 1, 2, 3 (and 4, the smooth conductor, with class 0; 6, the plastic, with class 2; 7, the roughplastic, with class 3: the classes only order the sort)
        w |= (cls & (MSK_N_CLASSES - 1u)) << MSK_CLASS_SHIFT;
        std::memcpy(&bvh.tris[k * 16 + 3], &w, 4);
    }
}

}  // namespace mskscene
