/*
 * msk_gpu.h — C ABI of the MI355X path-tracing back end for misaki-render.
 *
 * This is the drop-in boundary for ONE hot path of the reference:
 *
 *   SamplingIntegrator::render          src/librender/integrator.cpp:31-80
 *     -> render_block / render_sample   src/librender/integrator.cpp:82-126
 *     -> PathTracer::sample             src/librender/integrators/path.cpp:23-125
 *     -> Scene::ray_intersect/ray_test  src/librender/scene.cpp:216-273 (Embree3)
 *     -> ImageBlock::put / Film::put    src/librender/imageblock.cpp:36-114
 *
 * The reference has no FFI of its own (it is one C++ shared library); the entry
 * points below are what its `"path"` Integrator plugin
 * (include/misaki/render/integrator.h:9-17, integrators/path.cpp:139-140)
 * binds instead of running the Embree3+TBB tile loop.  INTEGRATION.md shows the
 * plugin-side stub.  Plain pointers and sizes only — no C++ or torch types.
 *
 * Conventions
 *   - every function returns MSK_OK (0) or a negative MSK_ERR_* code; the text
 *     of the last error is available from msk_gpu_last_error().  No exception
 *     crosses this boundary (the plugin turns a non-zero code into the
 *     reference's `Throw`, include/misaki/core/logger.h:81-88).
 *   - the caller owns every host array for the duration of the call that takes
 *     it; the library copies what it needs into HBM.
 *   - handles are opaque and destroyed explicitly.
 *   - one calling thread per msk_ctx at a time (the reference calls render()
 *     from a single worker thread, src/apps/main.cpp:37).  A render call drives
 *     four HIP streams of its own from the calling thread (MSK_HOST_THREADS=4:
 *     from three short-lived helper threads as well) and sleeps while the
 *     device works; every wait has a wall limit (MSK_WATCHDOG_S): the call
 *     returns, with MSK_ERR_HIP and a lost context if the device stopped
 *     answering.  The streams are created at the device's highest stream
 *     priority (MSK_STREAM_PRIORITY) so that they do not share hardware queues
 *     with the application's other streams.
 */
#ifndef MSK_GPU_H
#define MSK_GPU_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MSK_ABI_VERSION 8

/* ---- status codes ------------------------------------------------------- */
#define MSK_OK                 0
#define MSK_ERR_INVALID_ARG   (-1)
#define MSK_ERR_NO_DEVICE     (-2)
#define MSK_ERR_HIP           (-3)
#define MSK_ERR_OOM           (-4)
#define MSK_ERR_UNSUPPORTED   (-5)

/* ---- plugin type tags (the reference's registered plugin names) --------- */
#define MSK_BSDF_DIFFUSE        0  /* "diffuse"        bsdfs/diffuse.cpp:73          */
#define MSK_BSDF_ROUGHCONDUCTOR 1  /* "roughconductor" bsdfs/roughconductor.cpp:139 (GGX only) */
#define MSK_BSDF_ROUGHDIELECTRIC 2 /* "roughdielectric" bsdfs/roughdielectric.cpp:209 (GGX only) */
#define MSK_BSDF_DIELECTRIC     3  /* "dielectric"     bsdfs/dielectric.cpp:105 (smooth interface: two delta lobes) */
#define MSK_BSDF_CONDUCTOR      4  /* "conductor"      bsdfs/conductor.cpp (smooth metal: one delta reflection lobe; semantics at msk_bsdf_desc) */
#define MSK_BSDF_PLASTIC        6  /* "plastic": a smooth dielectric coat (one delta reflection lobe) over a diffuse base; semantics at
                                      msk_bsdf_desc.  Type 5 is unassigned and refused */
#define MSK_BSDF_ROUGHPLASTIC   7  /* "roughplastic": the plastic with a rough (GGX) coat in the delta one's place; semantics at msk_bsdf_desc */
#define MSK_EMITTER_AREA       0   /* "area"     emitters/area.cpp:61          */
#define MSK_TEXTURE_CHECKERBOARD 1 /* "checkerboard" textures/checkerboard.cpp:52 */
#define MSK_TEXTURE_BITMAP       2 /* "bitmap", bilinear filter (ABI v8; semantics below, at msk_texture_desc) */
#define MSK_TEXTURE_BITMAP_NEAREST 3 /* "bitmap", nearest-texel filter                                        */

#define MSK_EMITTER_CONSTANT   1   /* "constant" emitters/constant.cpp:95 (environment; mesh_id = -1, at most one) */
#define MSK_EMITTER_ENVMAP     2   /* "envmap": a lat-long radiance image, importance-sampled (environment; mesh_id = -1; at most one environment
                                      emitter per scene, `constant` or `envmap`; msk_envmap_desc + msk_gpu_scene_create_env below) */
#define MSK_EMITTER_POINT      3   /* "point" emitters/point.cpp: an isotropic delta light (mesh_id = -1; any number; its position comes in an
                                      msk_point_desc through msk_gpu_scene_create_ext; semantics at msk_point_desc below) */
#define MSK_EMITTER_SPOT       4   /* "spot": a point light times a cone factor (delta light; mesh_id = -1; any number; its geometry comes in an
                                      msk_light_desc through msk_gpu_scene_create_lights; semantics at msk_light_desc below) */
#define MSK_EMITTER_DIRECTIONAL 5  /* "directional": a sun, parallel light from one direction (delta light; mesh_id = -1; any number; its
                                      direction comes in an msk_light_desc, as for MSK_EMITTER_SPOT) */

/* AOV channel groups of the "aov" integrator (integrators/aov.cpp:21-28,87-144); channels per type: 1 3 2 3 3 4 */
#define MSK_AOV_DEPTH          0   /* si.t, 0 on a miss                                  (aov.cpp:97-99)   */
#define MSK_AOV_POSITION       1   /* si.p                                               (aov.cpp:101-105) */
#define MSK_AOV_UV             2   /* si.uv                                              (aov.cpp:107-110) */
#define MSK_AOV_GEO_NORMAL     3   /* si.n                                               (aov.cpp:112-116) */
#define MSK_AOV_SH_NORMAL      4   /* si.sh_frame.n                                      (aov.cpp:118-122) */
#define MSK_AOV_PATH_RGBA      5   /* nested "path" integrator: xyz_to_srgb(XYZ of its sample), 1 (aov.cpp:124-141) */

/* RNG semantics (the reference's own seeding is not reproducible) */
#define MSK_RNG_PCG_BLOCK      0   /* samplers/independent.cpp as written: one PCG32 stream per image block, drawn from in the scalar
                                      loops' order.  Sequential by construction: the device renders one block per LANE (msk_serial.h) —
                                      a fidelity mode (BASELINE config 1 in about 1.2 seconds, one block per wave), bit-identical to the oracle's; msk_gpu_render /
                                      _render_device only (not the "aov" integrator, not msk_gpu_sample_pixels) */
#define MSK_RNG_COUNTER        1   /* stateless hash of (seed,pixel,sample,dim): the hot path (wavefront kernels); GPU + oracle */

#define MSK_CIE_SAMPLES        95  /* include/misaki/core/spectrum.h:75        */
#define MSK_FILTER_RESOLUTION  32  /* include/misaki/render/rfilter.h:6        */

/*
 * One triangle mesh = one reference `Mesh` (include/misaki/render/mesh.h:86-90).
 * Vertices use the reference's interleaved layout, 8 floats per vertex
 * [px py pz nx ny nz u v] (shapes/obj.cpp:137-142), already in world space
 * (obj.cpp:90,102).  Faces are 3 uint32 per triangle, local to the mesh.
 * Mesh order == the reference's m_shapes order == Embree geomID (scene.cpp:235-240).
 */
typedef struct msk_mesh_desc {
    uint32_t first_vertex;   /* offset into msk_scene_desc.vertices, in vertices */
    uint32_t vertex_count;
    uint32_t first_face;     /* offset into msk_scene_desc.faces, in triangles  */
    uint32_t face_count;
    int32_t  bsdf_id;        /* index into bsdfs[]                              */
    int32_t  emitter_id;     /* index into emitters[], -1 = not an emitter      */
    uint32_t has_normals;    /* Mesh::has_vertex_normals()  (mesh.h:66)         */
    uint32_t has_texcoords;  /* Mesh::has_vertex_texcoords() (mesh.h:67)        */
} msk_mesh_desc;

/*
 * A tabulated spectrum on a regular wavelength grid = the reference's `regular` texture plugin
 * (spectra/regular.cpp:27-91,148 — what <spectrum value="l0:v0, l1:v1, ..."/> with equidistant
 * wavelengths becomes, xml.cpp:300-341; the loader has already multiplied the values of a spectrum inside an
 * <emitter> by MSK_CIE_Y_NORMALIZATION, xml.cpp:306-314).  value(l) = lerp of values[first_value + i], i = 0 .. size-1,
 * at x = (l - lambda_min) * inv_interval with inv_interval = float(1 / ((double) lambda_max - lambda_min) / (size - 1)))
 * and the segment index clamped to [0, size - 2] (RegularSpectrum::eval -> eval_pdf, regular.cpp:73-91: outside the
 * table the end segments are continued linearly).  ABI v7.  2 <= size <= MSK_REGULAR_MAX (the D65 and CIE tables'
 * 95; regular.cpp:30-31 needs two entries), lambda_min < lambda_max, values finite and non-negative (regular.cpp:59-60).
 * An `irregular` spectrum (unequal steps) is not part of this ABI: the host loader refuses it with its own message.
 */
#define MSK_REGULAR_MAX 95
typedef struct msk_regular_spectrum_desc {
    float    lambda_min, lambda_max;
    uint32_t size;
    uint32_t first_value;    /* offset into msk_scene_desc.regular_values       */
} msk_regular_spectrum_desc;

/* A spectrum the device can evaluate.  regular == 0: value(l) = scale * S(coeff, l) with the sigmoid polynomial
 * S of render/srgb.h:8-19; RGB triples above 1 use the normalisation of srgb_d65.cpp:18-22
 * (scale = 2 * max(rgb), coeff = fetch(rgb / scale)) without the D65 factor; scale >= 0.
 * regular == k > 0 (ABI v7): the tabulated spectrum regular_spectra[k - 1] of the scene; coeff / scale are ignored. */
typedef struct msk_spectrum_desc {
    float coeff[3];
    float scale;
    uint32_t regular;
} msk_spectrum_desc;

/*
 * BSDF parameters.
 * MSK_BSDF_DIFFUSE: `reflectance` = the three sigmoid-polynomial coefficients srgb_model_fetch()
 * returned for the RGB reflectance (spectra/srgb.cpp:13-19, srgb.cpp:11-28).
 * MSK_BSDF_ROUGHCONDUCTOR (bsdfs/roughconductor.cpp:12-50): GGX microfacet conductor; alpha_u/alpha_v,
 * sample_visible, and eta / k / specular_reflectance evaluated at the path's four wavelengths (the
 * reference's RGB-typed code does not compile in its spectral build; DESIGN.md §rough conductor).
 * MSK_BSDF_ROUGHDIELECTRIC (bsdfs/roughdielectric.cpp:14-55): GGX microfacet dielectric with reflection and
 * transmission lobes; ior_eta = int_ior / ext_ior, ior_inv_eta = ext_ior / int_ior, alpha_*, sample_visible,
 * specular_reflectance / specular_transmittance.
 * MSK_BSDF_DIELECTRIC (bsdfs/dielectric.cpp:13-72): smooth dielectric interface, a delta reflection and a delta
 * transmission lobe chosen by the Fresnel reflectance (render/fresnel.h:37-63); ior_eta / ior_inv_eta and
 * specular_reflectance / specular_transmittance as for MSK_BSDF_ROUGHDIELECTRIC (the reference's defaults: int_ior 1.49,
 * ext_ior 1.00028); alpha_* and sample_visible are ignored.  eval and pdf are zero: no next-event sample is taken at such a
 * hit (path.cpp:56) and the emitter the sampled ray reaches counts with MIS weight 1 (path.cpp:104-106).  back_bsdf must be
 * -1 (twosided.cpp:33-35: no transmission under "twosided").
 * MSK_BSDF_CONDUCTOR (bsdfs/conductor.cpp, whose RGB-typed code is not built; evaluated at the path's four wavelengths, like
 * MSK_BSDF_ROUGHCONDUCTOR): a smooth conductor, one delta reflection lobe.  It reads eta, k, specular_reflectance and back_bsdf;
 * alpha_*, sample_visible and reflectance* are ignored; ior_eta / ior_inv_eta are 1 / 1 (or 0 / 0, unset): a conductor has no
 * relative index, and a type-4 descriptor that carries one (a descriptor of another kind with its type overwritten — type 4 was
 * unassigned before) is refused with MSK_ERR_INVALID_ARG, "type 4 is not supported for a descriptor with ...".  sample: cos_i = wi.z; cos_i <= 0 fails (no direction); otherwise
 * wo = (-wi.x, -wi.y, wi.z), pdf = 1, eta = 1, value(l) = specular_reflectance(l) * fresnel_conductor(cos_i, eta(l), k(l))
 * (render/fresnel.h, fp32 as msk_device.h has it; one product).  eval and pdf are zero: no next-event sample is taken at such a
 * hit and the emitter the sampled ray reaches counts with MIS weight 1, as for MSK_BSDF_DIELECTRIC.  Under "twosided" (back_bsdf
 * = its own index) it mirrors on both faces; one-sided (back_bsdf = -1) it is black from behind.  The reference's defaults,
 * which the flatteners write when a parameter is absent, are eta = 0, k = 1, specular_reflectance = 1 (uniform spectra): for them
 * fresnel_conductor is exactly 1.0f for every cos_i in (0, 1], a perfect mirror.
 * MSK_BSDF_PLASTIC (bsdfs/roughplastic.cpp with a delta coat in the GGX coat's place; Mitsuba's `plastic`): a delta reflection lobe
 * and a diffuse lobe, one of them picked per sample.  It reads the diffuse reflectance rho(l) exactly as MSK_BSDF_DIFFUSE does
 * (reflectance, reflectance_scale, reflectance_texture, reflectance_regular), specular_reflectance = a constant spectrum s(l),
 * ior_eta = int_ior / ext_ior and ior_inv_eta, sample_visible read as `nonlinear` (0, or anything else = 1) and back_bsdf; alpha_*,
 * eta, k and specular_transmittance are ignored.  An ior_eta that is not finite or is below 1 is refused.  Two constants per entry
 * are computed at scene creation, in double, and rounded to fp32 (msk_gpu_plastic_constants returns them):
 *   fdr_int = 1 - (1 - fdr_ext) / ior_eta^2, fdr_ext = 2 * integral over mu in [0, 1] of F(mu; ior_eta) mu (Gauss-Legendre), F the
 *             exact unpolarised dielectric Fresnel reflectance: the hemispherical reflectance seen from inside;
 *   ssw     = s_mean / (d_mean + s_mean), the means of s(l) and of rho(l) over the 95 CIE sample wavelengths (a bitmap: over its
 *             texels too; a checkerboard: over its two colours); 1 when both means are 0.  It moves variance only.
 * fp32, one operation at a time, with wi on the front side: cos_i = wi.z, F_i = fresnel_dielectric(cos_i, ior_eta) (render/fresnel.h:37-63
 * as msk_device.h has it), ps = F_i * ssw, pd = (1 - F_i) * (1 - ssw).  cos_i <= 0 or ps + pd == 0: the sample fails, eval and
 * pdf are 0.  Otherwise ps = ps / (ps + pd), pd = 1 - ps, and D(l) = rho(l) / (1 - fdr_int * rho(l)) when nonlinear, else
 * rho(l) / (1 - fdr_int).  sample: sample1 < ps takes the delta lobe, wo = (-wi.x, -wi.y, wi.z), pdf = ps, value(l) = s(l) * F_i / ps,
 * eta = 1.  Otherwise the diffuse lobe: wo = square_to_cosine_hemisphere(u), F_o = fresnel_dielectric(wo.z, ior_eta), pdf =
 * pd * wo.z / pi (as pd * (1 / pi * wo.z)), value(l) = D(l) * ior_inv_eta^2 * (1 - F_i) * (1 - F_o) / pd, and 0 when pdf <= 0; eta = 1.
 * eval and pdf are the diffuse lobe's alone, for cos_i > 0 and cos_o > 0: eval(l) = D(l) * ior_inv_eta^2 * (1 - F_i) * (1 - F_o) *
 * (1 / pi) * cos_o, pdf = pd * (1 / pi * cos_o).  The products run left to right as written, with f = ior_inv_eta * ior_inv_eta *
 * (1 - F_i) * (1 - F_o) one scalar.  Integrator: a plastic hit always takes its next-event sample; when the sampled lobe is the
 * delta one the emitter the ray reaches counts with emitter density 0, MIS weight 1 (path.cpp:104-106), as after a mask's null lobe.
 * A scene that holds one runs the kernels a `mask` scene runs (every entry then has a mask record, the constant opacity 1 unless the
 * scene gives it a mask), `mask` over it is allowed, and the "direct" integrator refuses it (MSK_ERR_UNSUPPORTED).
 * MSK_BSDF_ROUGHPLASTIC (bsdfs/roughplastic.cpp, which is RGB-typed and not built: this text is the specification): the plastic with
 * a GGX coat in the delta one's place, two smooth lobes.  It reads what MSK_BSDF_PLASTIC reads, with the same refusals and the same
 * two constants fdr_int and ssw, and alpha_u: alpha_v must equal it ("anisotropic" coats are refused, MSK_ERR_INVALID_ARG, as
 * roughplastic.cpp:23-25 does), a negative or non-finite alpha is refused, and a = max(alpha_u, 1e-4) is applied at use, as for the
 * rough types.  sample_visible is read as `nonlinear`, as for the plastic.  Departure: there is no visible-normal variant.  The
 * reference's MicrofacetDistribution::sample (render/microfacet.h:131-143) draws the normal from D(m) cos(theta_m) whatever the flag,
 * while roughplastic.cpp:144-146 returns the visible-normal density under it, so that sample = eval / pdf is biased there; the
 * reference's default is false (microfacet.h:53,90), for which the file is consistent, and that is what is built.
 * fp32, one operation at a time, wi on the front side: cos_i = wi.z; F_i, ps, pd and their failure conditions exactly as for the
 * plastic.  eval / pdf for cos_i > 0 and cos_o > 0 (0 otherwise, and where the plastic's lobes fail): H = normalized(wo + wi), D =
 * distr_eval(H, a, a), G = smith_g1(wi, H, a, a) * smith_g1(wo, H, a, a), F_h = fresnel_dielectric(dot(wi, H), ior_eta), c =
 * ((F_h * D) * G) / (4 * cos_i), base(l) = the plastic's eval(l), value(l) = s(l) * c + base(l); p_s = (D * H.z) / (4 * dot(wo, H)),
 * 0 when D == 0; pdf = ps * p_s + pd * ((1 / pi) * cos_o).  sample: sample1 < ps draws m = sample_ggx(u, a, a, &pm) (the function
 * the roughconductor calls) and wo = m * 2 * dot(wi, m) - wi; pm == 0 or wo.z <= 0: a direction was produced, value 0, pdf 0.
 * Otherwise wo = square_to_cosine_hemisphere(u).  Then pdf = pdf(wi, wo), value = pdf > 0 ? eval(wi, wo) / pdf : 0
 * (roughplastic.cpp:71-75); eta = 1; the sample is never delta.  Integrator: an ordinary smooth BSDF — every hit takes its next-event
 * sample with this eval / pdf, an emitter the sampled ray reaches is weighted with the mixture pdf.  A scene that holds one runs
 * the kernels a plastic scene runs, `mask` over it is allowed, and the "direct" integrator refuses it (MSK_ERR_UNSUPPORTED).
 * back_bsdf implements the "twosided" adapter (bsdfs/twosided.cpp:38-101): the BSDF evaluated with
 * flipped wi/wo when cos(theta_i) < 0; the entry's own index for twosided(A), -1 for a one-sided BSDF.
 * reflectance_texture: 0 = the diffuse reflectance is the constant `reflectance`; k > 0 = it is
 * textures[k-1] evaluated at the hit's uv (SmoothDiffuse::m_reflectance->eval(si), diffuse.cpp:31,44).
 */
typedef struct msk_bsdf_desc {
    int32_t type;
    int32_t back_bsdf;
    float   reflectance[3];
    float   alpha_u, alpha_v;
    int32_t sample_visible;
    msk_spectrum_desc eta, k, specular_reflectance, specular_transmittance;
    float   ior_eta, ior_inv_eta;
    uint32_t reflectance_texture;
    float   reflectance_scale;   /* diffuse reflectance = S(reflectance, l) * reflectance_scale: 1 for an `srgb` spectrum; a
                                    `uniform` spectrum of value c (spectra/uniform.cpp:16-27, what <spectrum value="c"/> makes
                                    outside an emitter, xml.cpp:285-292) is {0, 0, +inf} with scale c */
    uint32_t reflectance_regular; /* ABI v7: k > 0 = the diffuse reflectance is the tabulated spectrum regular_spectra[k - 1]
                                    (reflectance / reflectance_scale / reflectance_texture are then unused); 0 = not tabulated */
} msk_bsdf_desc;

/*
 * A texture that varies over the surface.  MSK_TEXTURE_CHECKERBOARD (textures/checkerboard.cpp:10-33):
 * uv' = m_transform.transform_affine_point(si.uv) with m_transform = the top-left 3x3 of the `to_uv`
 * 4x4 (Transform4f::extract, core/transform.h:142-148; `to_uv` holds its rows 0 and 1, so the uv offset
 * is the 4x4's z column), u = uv'.x - floor(uv'.x), v likewise; color0 where (u > .5) == (v > .5), else
 * color1.  color0 / color1 are sigmoid-polynomial coefficients of two constant `srgb` spectra (nested
 * textures other than that are not flattened).  si.uv = the interpolated vertex texcoords, or the
 * hit's barycentrics for a mesh without them (mesh.cpp:66,68-72).
 *
 * MSK_TEXTURE_BITMAP / MSK_TEXTURE_BITMAP_NEAREST (ABI v8): an image of width x height texels, texels[first_texel ..] of the
 * scene, row-major, row 0 first; a texel holds the three sigmoid-polynomial coefficients srgb_model_fetch() returned for its
 * linear-sRGB colour (components clamped to [0, 1] first: a reflectance).  Texel row j covers v in [j/H, (j+1)/H), column i
 * covers u in [i/W, (i+1)/W).  (The reference's textures/bitmap.cpp is RGB-typed and not built; this is its lookup in the
 * spectral form.)  With uv' as above, fu = uv'.x - floor(uv'.x) (wrap = repeat; fu can be exactly 1 for a tiny negative uv'.x),
 * all in fp32, one operation at a time:
 *   nearest:  i = min((int) (fu * W), W - 1), j likewise; value(l) = S(texel[j][i], l)
 *   bilinear: px = fu * W - 0.5; i0 = (int) floor(px); tx = px - i0; i0 < 0 -> W - 1; i0 >= W -> 0; i1 = i0 + 1, i1 >= W -> 0
 *             (the same in y); s00 .. s11 = S(texel[j0|j1][i0|i1], l); a = s00 + tx (s10 - s00); b = s01 + tx (s11 - s01);
 *             value = a + ty (b - a): spectral VALUES are interpolated, not coefficients.
 * color0 / color1 are ignored for a bitmap.
 */
typedef struct msk_texture_desc {
    int32_t type;
    float   color0[3];
    float   color1[3];
    float   to_uv[6];        /* m00 m01 m02 / m10 m11 m12 */
    uint32_t width, height;  /* bitmap: texels per row, rows (>= 1)                             */
    uint32_t first_texel;    /* bitmap: offset into msk_scene_desc.texels, in texels            */
} msk_texture_desc;

/*
 * Area emitter (emitters/area.cpp) with an `srgb_d65` radiance
 * (spectra/srgb_d65.cpp:13-36): radiance(l) = d65(l) * d65_scale * S(coeff, l),
 * d65_scale = scale * 2*max(rgb) / 10568 (srgb_d65.cpp:18-26, d65.cpp:33-34).
 * The constant environment emitter (emitters/constant.cpp) uses the same radiance form (its default is
 * Texture::D65(1): coefficients {0, 0, +inf}); it has no mesh (mesh_id = -1), and its place in `emitters`
 * is its place in Scene::m_emitters (scene.cpp:27-41: XML order, shapes' area lights and top-level emitters mixed).
 */
typedef struct msk_emitter_desc {
    int32_t type;
    int32_t mesh_id;         /* the shape this emitter is attached to          */
    float   radiance[3];     /* sigmoid-polynomial coefficients                */
    float   d65_scale;
    uint32_t radiance_regular; /* ABI v7: k > 0 = radiance(l) is the tabulated spectrum regular_spectra[k - 1] as it stands
                                  (AreaLight / ConstantBackgroundEmitter with a `regular` radiance: no D65 factor, no
                                  sigmoid; radiance / d65_scale unused); 0 = the srgb_d65 form above */
} msk_emitter_desc;

/*
 * The image of an MSK_EMITTER_ENVMAP emitter.  Its msk_emitter_desc has mesh_id = -1, radiance = {0, 0, +inf}, d65_scale =
 * scale / 10568 and radiance_regular = 0: the emitter's own table T_e(l) = d65(l) * d65_scale, as for every srgb_d65 radiance.
 * (The reference's emitters/envmap.cpp is RGB-typed and not built; kept from it: the lat-long convention, dist = 2 * radius, the
 * Jacobian 1 / (2 pi^2 sin theta), to_world applied to directions.  Not kept: core/distribution.h's Distribution2D and
 * path.cpp's stale records on an environment hit)  Everything below is fp32, one operation at a time.
 *
 * Radiance.  width x height texels, row-major, row 0 = the image's top row = theta near 0.  A texel of linear RGB c >= 0 is
 * {c0, c1, c2, w}: the coefficients srgb_model_fetch(c / (2 max c)) and the factor w = 2 max c, the srgb_d65 flattening; a black
 * texel is {0, 0, 0, 0}.  L(u, v, l) = T_e(l) * bilerp_k(w_k * S(coeff_k, l)) with the bilinear form of MSK_TEXTURE_BITMAP
 * (px = u * W - 0.5, ..., a + t (b - a): spectral VALUES are interpolated), except that v CLAMPS at the poles (j0 < 0 -> 0,
 * j1 >= H -> H - 1) while u wraps.
 *
 * Direction to uv.  dl = R^T d with R = to_world (row-major 3x3; must be a rotation: |R R^T - 1| <= 1e-4 per entry and
 * det > 0, anything else is refused).  u = atan2(dl.x, -dl.z) / (2 pi), then u - floor(u) (a result of 1 becomes 0);
 * v = atan2(sqrt(dl.x^2 + dl.z^2), dl.y) / pi.  atan2(y, x) = x == 0 ? (y > 0 ? pi/2 : y < 0 ? -pi/2 : 0) : det_atan(y / x)
 * (+ pi for x < 0 and y >= 0, - pi for x < 0 and y < 0); pi and 2 pi are the fp32 constants.  uv to direction:
 * theta = pi v, phi = 2 pi u, (st, ct) = det_sincos(theta), (sp, cp) = det_sincos(phi), dl = (sp st, ct, -cp st), d = R dl.
 *
 * Distribution.  Piecewise constant over the texels from the host's weights (one per texel, finite, >= 0, not all zero; the
 * host plugin supplies (sum of the luminance of the 3x3 neighbourhood, u wrapped, v clamped) * sin(pi (j + .5) / H), which is
 * positive wherever the bilinear lookup is).  The library builds, in double and stored as float, per row a cumulative table of
 * W + 1 entries (0 .. 1; a row of zero weight is 0 .. 0 1) and the marginal of H + 1 entries over the row sums.
 * Sampling (u.x, u.y): row j from u.y in the marginal, then column i from u.x in row j, both by the upper-bound search + clamp
 * + sample_reuse of core/distribution.h:106-116; the reused fractions dv, du are clamped to <= 1 - 2^-24;
 * uv = ((i + du) / W, (j + dv) / H) (either can still round up to 1: the lookup wraps u and clamps v); p(uv) = (marg[j+1] - marg[j]) * (cond[j][i+1] - cond[j][i]) * (float) W * (float) H;
 * sin theta = sqrt(max(dl.x^2 + dl.z^2, eps^2)) with eps = 2^-24; pdf_omega = p / (2 pi^2 sin theta) (2 pi^2 = 2 * (pi * pi) in fp32).
 * pdf(direction): uv as above, i = min((int) (u W), W - 1), j likewise, the same product.  For a direction the sampler produced
 * this is the number the sampler returned, bit for bit, when to_world is the identity (R^T (R dl) is then dl exactly) and the
 * direction comes back into the cell it was drawn from; it does not when uv lies within the few 2^-24 of a cell border that
 * det_sincos, the rotation and det_atan move it by (tests/envmap_ref.py: the excluded case, below 0.1 % of random numbers).
 * Under a rotation R^T (R dl) differs from dl by three roundings per component, 2^-22 absolute on sin theta: the two numbers then
 * agree within 2^-21 / sin theta + 2^-21 relative.  Next-event value = L(uv) / pdf_omega,
 * dist = 2 * env_radius; pdf 0 gives no contribution.  On the miss branch the value is L(ray direction) and the emitter density
 * of the MIS weight pdf(ray direction) / n_emitters (0 after a delta lobe).
 */
typedef struct msk_envmap_desc {
    uint32_t width, height;
    const float *texels;     /* width * height * 4: c0 c1 c2 w */
    const float *weights;    /* width * height                 */
    float to_world[9];       /* row-major rotation             */
} msk_envmap_desc;

/*
 * The position of an MSK_EMITTER_POINT emitter (emitters/point.cpp).  Its msk_emitter_desc has mesh_id = -1 and holds the
 * INTENSITY I(l) (W / sr per nm) in radiance / d65_scale / radiance_regular, in the two forms every emitter's radiance has; its
 * index in `emitters` is its place in Scene::m_emitters (XML order, scene.cpp:27-41).  Exactly one msk_point_desc per such
 * emitter, in any order.  Everything below is fp32, one operation at a time, IEEE sqrt and division, no contraction.
 *
 * Next-event sample from a reference point p:  d = position - p;  dist = sqrt(d.x d.x + (d.y d.y + d.z d.z));  inv = 1 / dist;
 * d = d * inv;  pdf = 1;  value(l) = (I(l) * inv) * inv.  dist == 0 gives pdf = 0 and no contribution.  The two random numbers of
 * the bounce are drawn and, with several emitters, u.x is rescaled as for every emitter; selection is the existing one
 * (pdf *= 1 / n, value *= n).  The shadow ray is the existing one: direction d, length dist * (1 - MSK_SHADOW_EPS).
 * Not kept from path.cpp as written: the reference would weight this sample mis_weight(1, bsdf_pdf); a delta emitter cannot be
 * reached by a BSDF sample, so that weight loses energy.  Here the next-event term is thr * value * bsdf_val, weight 1
 * (DESIGN.md section 9).  A point light is never hit or seen: no term at depth 1, no emitter density for a BSDF sample, and
 * hide_emitters does not concern it.  It may lie outside the scene's bounds and does not switch the camera cull off.
 *
 * In a scene that holds a point emitter or an MSK_BSDF_CONDUCTOR (the kernels with these branches), a `constant` environment hit
 * by a BSDF sample counts with the emitter density of the ray's own direction, (1 / 4 pi) / n_emitters, or 0 after a delta lobe:
 * the rule MSK_EMITTER_ENVMAP follows.  (The older kernels keep path.cpp's stale next-event record there; with a point light that
 * record holds no density and the two weights would no longer sum to 1.)
 */
typedef struct msk_point_desc {
    uint32_t emitter;        /* index into msk_scene_desc.emitters: an MSK_EMITTER_POINT entry */
    float    position[3];    /* world space, finite                                            */
} msk_point_desc;

/* What a scene holds beyond msk_scene_desc (whose layout is fixed by ABI v8): the envmap emitter's image (or NULL) and the
   point emitters' positions (n_points may be 0, points then unused). */
typedef struct msk_scene_ext {
    const msk_envmap_desc *envmap;
    uint32_t n_points;
    const msk_point_desc *points;
} msk_scene_ext;

/*
 * The `mask` BSDF (bsdfs/mask.cpp): an opacity cutout with a null lobe, as a decoration of ONE entry of msk_scene_desc.bsdfs (at most
 * one msk_mask_desc per entry).  Let a be the opacity at the hit's uv, a scalar in [0, 1], and X the nested BSDF: the entry itself
 * with its back_bsdf flip.  The opacity read is always that of the entry the mesh names, taken before the twosided flip.
 * Everything below is fp32, one operation at a time, IEEE division, no contraction.
 *
 * Opacity.  filter 0: the constant `opacity`.  filter 1 / 2: an image of width x height scalars (row-major, `values`), looked up as
 * MSK_TEXTURE_BITMAP_NEAREST / MSK_TEXTURE_BITMAP look their texels up, word for word (msk_texture_desc: to_uv, repeat wrap, the
 * bilinear v = a0 + t (a1 - a0) on the values), the scalar standing where S(texel, l) stands.  An image of equal values is therefore
 * the constant, to the bit.  A value (or the constant) outside [0, 1] or not finite is refused at scene creation.
 *
 * sample(sample1, u): the lobe is picked by u.x (mask.cpp:43-44), not by sample1.  u.x < a: u.x = u.x / a, then X.sample(sample1, u)
 * with pdf = a * pdf_X and X's value.  Otherwise the null lobe: the continuation ray has the incoming ray's own world direction, bit
 * for bit (no frame round trip: interpolated shading frames are not orthonormal), pdf = 1 - a, value 1, eta = 1, and the lobe is
 * delta.  The null lobe is taken on either face: it does not see the cos_i <= 0 failure of a one-sided X.  a = 0 never samples X;
 * a = 1 never samples the null lobe, and there u.x / 1 and 1 * pdf are exact: the decorated entry is X to the bit.
 * eval = a * eval_X, pdf = a * pdf_X.
 *
 * Integrator ("path").  The next-event sample is taken iff X has a smooth lobe (path.cpp:56: flags, not the sampled lobe).  "The
 * last bounce was delta" (emitter density 0, MIS weight 1) holds when the null lobe was taken or X is delta.  Shadow rays are
 * unchanged: as in the reference (scene.cpp:91-95) a masked surface is opaque to them, and light through a cutout arrives by the
 * BSDF sample alone, with weight mis_weight(1 - a, 0) = 1.  A null bounce counts a depth and takes Russian roulette like any other;
 * the random numbers of a bounce are every BSDF's.  `scattered` (path.cpp:31,73) is false at the camera and true after any non-null
 * sample; under hide_emitters an emitter reached while it is still false adds nothing — the environment (path.cpp:92-93) and,
 * unlike path.cpp:82-88, an area emitter too.  A `constant` sky counts with the density of the ray's own direction, as in every
 * scene that runs the kernels of msk_point_desc.
 * Not kept from mask.cpp as written (departures 6-8): mask.cpp:47,53,68 multiplies the nested value by the
 * opacity AND returns the nested pdf unscaled (the nested lobe then carries a^2); the opacity is a scalar (the hosts reduce a colour
 * to 0.212671 r + 0.715160 g + 0.072169 b); the area emitter behind a cutout under hide_emitters.
 * "aov" renders see a masked surface as a surface: the primary-hit channels are those of the first hit, whatever its opacity.
 * The "direct" integrator refuses a scene that holds a mask (MSK_ERR_UNSUPPORTED): a cutout would be a black hole in it.
 */
typedef struct msk_mask_desc {
    uint32_t bsdf;           /* index into msk_scene_desc.bsdfs: the decorated entry                 */
    float    opacity;        /* filter 0: the constant, in [0, 1]                                    */
    int32_t  filter;         /* 0 constant, 1 nearest, 2 bilinear                                    */
    float    to_uv[6];       /* filter 1 / 2: row-major 2 x 3, as msk_texture_desc::to_uv            */
    uint32_t width, height;  /* filter 1 / 2: at least 1 x 1                                         */
    const float *values;     /* filter 1 / 2: width * height scalars in [0, 1], row 0 first          */
} msk_mask_desc;

/* msk_scene_ext is passed by pointer without a size and cannot grow in place: what a scene holds beyond it wraps it. */
typedef struct msk_scene_masks {
    msk_scene_ext ext;       /* the envmap emitter's image and the point emitters' positions, as above */
    uint32_t n_masks;        /* may be 0, masks then unused                                            */
    const msk_mask_desc *masks;
} msk_scene_masks;

/*
 * The geometry of an MSK_EMITTER_SPOT or MSK_EMITTER_DIRECTIONAL emitter: the two other delta lights.  The reference has neither
 * plugin; the semantics are this back end's own and are fixed here.  The emitter's msk_emitter_desc has mesh_id = -1 and keeps its
 * spectrum in radiance / d65_scale / radiance_regular, as MSK_EMITTER_POINT does: for a spot the PEAK INTENSITY I(l) (W / sr per nm),
 * for a sun the IRRADIANCE E(l) (W / m^2 per nm) on a surface that faces it.  Exactly one msk_light_desc per such emitter, in any
 * order.  Everything below is fp32, one operation at a time, IEEE sqrt and division, no contraction; dot products associate as
 * x x + (y y + z z).
 *
 * Spot, from a reference point p, with a = direction (the axis):  d, dist, inv exactly as at msk_point_desc (dist == 0 gives
 * pdf = 0);  c = -(d.x a.x + (d.y a.y + d.z a.z));  the falloff f, tested in this order:  c >= cos_beam gives 1;  c <= cos_cutoff
 * gives 0;  otherwise t = (c - cos_cutoff) / (cos_beam - cos_cutoff) and f = (t * t) * (3.f - 2.f * t).
 * value(l) = ((I(l) * inv) * inv) * f, pdf = 1;  f == 0 gives pdf = 0: no contribution and no shadow ray.  (A smoothstep in cosine
 * space, as in pbrt-v4, not Mitsuba's ramp in angle: no inverse trigonometry on the device, and it can be restated exactly.
 * cos_cutoff == cos_beam is a hard edge.  With cos_cutoff = cos_beam = -1 the first branch is taken wherever c is a number and
 * the spot is the point light, to the bit.)
 *
 * Directional, with w = direction:  d = (-w.x, -w.y, -w.z);  dist = 2.f * env_radius, the radius of the sphere around the scene that
 * an environment emitter gets (a scene with a sun computes it whether it holds an environment emitter or not);  pdf = 1;
 * value(l) = E(l).
 *
 * For both, everything msk_point_desc says holds: the bounce's two random numbers are drawn, u.x is rescaled with several
 * emitters, selection is the existing one; the shadow ray is d with length dist * (1 - MSK_SHADOW_EPS); the next-event term has
 * weight 1 in "path" and in "direct"; the light is never hit or seen, has no emitter density for a BSDF sample, hide_emitters does
 * not concern it and it does not switch the camera cull off.  The scene runs the kernels of msk_point_desc, so a `constant` sky
 * follows the rule stated there.
 * Refused at scene creation (MSK_ERR_INVALID_ARG, the message names the emitter or the descriptor): a spot or sun without its
 * descriptor or with two, a descriptor whose emitter is of another type or out of range, n_lights without lights, a position
 * (spot) or direction that is not finite, | |direction|^2 - 1 | > 1e-5, cos_cutoff outside [-1, 1), cos_beam outside
 * [cos_cutoff, 1], mesh_id != -1.
 */
typedef struct msk_light_desc {
    uint32_t emitter;        /* index into msk_scene_desc.emitters: an MSK_EMITTER_SPOT or MSK_EMITTER_DIRECTIONAL entry   */
    float    position[3];    /* spot: world space, finite.  directional: ignored                                          */
    float    direction[3];   /* the way the light TRAVELS (spot: its axis), unit length, finite                           */
    float    cos_cutoff;     /* spot: cosine of the half-angle beyond which it is dark, in [-1, 1)                        */
    float    cos_beam;       /* spot: cosine of the half-angle inside which it is at full intensity,
                                cos_cutoff <= cos_beam <= 1                                                               */
} msk_light_desc;

/* msk_scene_masks cannot grow in place either: the spot and directional emitters' geometry wraps it. */
typedef struct msk_scene_lights {
    msk_scene_masks masks;   /* everything above                                                       */
    uint32_t n_lights;       /* may be 0, lights then unused                                           */
    const msk_light_desc *lights;
} msk_scene_lights;

/* PerspectiveCamera (sensors/perspective.cpp:8-42); matrices are row-major 4x4. */
typedef struct msk_camera_desc {
    float sample_to_camera[16];  /* m_sample_to_camera, sample space in PIXELS */
    float to_world[16];          /* m_world_transform                          */
    float near_clip, far_clip;
} msk_camera_desc;

/*
 * The `thinlens` sensor: the perspective camera with a lens of radius aperture_radius focused at the distance focus_distance along
 * the optical axis (sensors/thinlens.cpp of the Mitsuba family; the reference has no such plugin, the semantics are fixed here).
 * A scene created with an msk_lens_desc generates every camera ray as follows; a scene without one is the pinhole camera it always
 * was.  Everything is fp32, one operation at a time, IEEE division and square root, no contraction.  Inputs: the film position
 * (px, py) in pixels, the aperture sample u = counter_pair(key, 2) of the sample's key (pair 2 was reserved for it: no other random
 * number of a sample moves), R = aperture_radius, f = focus_distance, and msk_camera_desc.
 *   1. near_p: as the pinhole computes it.  r[q] = ((s2c[q][0] px + s2c[q][1] py) + s2c[q][2] 0) + s2c[q][3] 1 for the four rows q
 *      of sample_to_camera; near_p = (r[0] / r[3], r[1] / r[3], r[2] / r[3]).
 *   2. the lens point: (lx, ly) = square_to_uniform_disk_concentric(u) * R, one multiplication per component.  The map (core/warp.h):
 *      x = 2 u.x - 1, y = 2 u.y - 1;  x == 0 and y == 0: r = phi = 0;  x x > y y: r = x, phi = (pi / 4) (y / x);  otherwise r = y,
 *      phi = pi / 2 - (x / y) (pi / 4);  the point is (r cos phi, r sin phi) with the library's deterministic sine and cosine.
 *   3. the focus point: ft = f / near_p.z;  fp = (near_p.x ft, near_p.y ft, near_p.z ft).
 *   4. dl = normalized((fp.x - lx, fp.y - ly, fp.z)): v / sqrt(x x + (y y + z z));  inv_z = 1 / dl.z;  tnear = near_clip inv_z;
 *      tfar = far_clip inv_z.
 *   5. the origin: to_world applied to the point (lx, ly, 0), each row ((m[q][0] lx + m[q][1] ly) + m[q][2] 0) + m[q][3] 1, the
 *      first three divided by the fourth.
 *   6. the direction: to_world applied to dl as a vector, m[q][0] dl.x + (m[q][1] dl.y + m[q][2] dl.z), as the pinhole does.
 * The ray's weight stays 1 (an ideal thin lens, no vignetting).  aperture_radius = 0 is valid and goes through this code: the origin
 * is then the pinhole's (bit for bit wherever a coordinate of it is not zero; a zero may differ in its sign); the direction goes
 * through f / near_p.z and back and may differ from the pinhole's in its last bits.
 * Refused at scene creation (MSK_ERR_INVALID_ARG, the message names the field): aperture_radius negative, NaN or infinite;
 * focus_distance not finite or not greater than 0.
 * A scene with a lens runs kernels of its own (k_shade_gen_l, k_wavefront_l, k_wavefront_h_l; "direct": k_direct<*, true>), whatever
 * else it holds; every other scene runs the kernels it ran before.  MSK_RNG_PCG_BLOCK renders of a scene with a lens are refused
 * (MSK_ERR_UNSUPPORTED, the message names the sensor): the reference's sampler draws no aperture sample that could pin that mode.
 */
typedef struct msk_lens_desc {
    float aperture_radius;   /* R >= 0, finite, in camera-space units      */
    float focus_distance;    /* f > 0, finite: the plane z = f is in focus */
} msk_lens_desc;

/* msk_scene_lights cannot grow in place either: the lens wraps it. */
typedef struct msk_scene_lens {
    msk_scene_lights lights;     /* everything above                                   */
    const msk_lens_desc *lens;   /* NULL: the pinhole camera of msk_camera_desc alone  */
} msk_scene_lens;

/* Film::size() (film.cpp:10) + ReconstructionFilter discretisation (rfilter.cpp:12-27) + the crop window
 * (film.cpp:12-21,51-63: crop_offset_x / _y, crop_width / _height; HDRFilm's storage is an ImageBlock of the
 * crop size placed at the crop offset, films/hdrfilm.cpp:37-38).  The sensor — sample_to_camera, the pixel
 * grid, the spiral block ids — is that of the FULL film (integrator.cpp:45: BlockGenerator(film->size(), 0,
 * block_size)); the film the render calls write is the crop window, crop_size[1] x crop_size[0] pixels, and
 * holds exactly what Film::put leaves there: every block's contribution clipped to the window
 * (imageblock.cpp:36-53,133-173).  Blocks whose bordered area misses the window add nothing and are not
 * rendered (and not counted in msk_stats).  crop_size = {0, 0} means the whole film. */
typedef struct msk_film_desc {
    int32_t width, height;
    float   filter_radius;                       /* m_radius                    */
    float   filter_lut[MSK_FILTER_RESOLUTION + 1]; /* m_values, [32] == 0       */
    int32_t crop_offset[2];                      /* m_crop_offset (x, y)        */
    int32_t crop_size[2];                        /* m_crop_size (width, height) */
} msk_film_desc;

typedef struct msk_scene_desc {
    uint32_t abi_version;       /* MSK_ABI_VERSION                             */
    uint32_t n_meshes, n_bsdfs, n_emitters;
    const msk_mesh_desc    *meshes;
    const msk_bsdf_desc    *bsdfs;
    const msk_emitter_desc *emitters;
    const float    *vertices;   /* n_vertices * 8 floats                       */
    const uint32_t *faces;      /* n_faces * 3                                 */
    uint32_t n_vertices, n_faces;
    msk_camera_desc camera;
    msk_film_desc   film;
    /* spectral tables owned by the host side of the reference
       (spectrum.cpp:8-111: x,y,z each 95 samples 360..830 nm; d65.cpp:12-27) */
    const float *cie1931_xyz;   /* 3 * MSK_CIE_SAMPLES                         */
    const float *d65;           /* MSK_CIE_SAMPLES                             */
    uint32_t n_textures;        /* may be 0 (textures then unused)             */
    const msk_texture_desc *textures;
    /* ABI v7: tabulated spectra (may be 0 / NULL) */
    uint32_t n_regular_spectra, n_regular_values;
    const msk_regular_spectrum_desc *regular_spectra;
    const float *regular_values;
    /* ABI v8: the texel pool of the bitmap textures (may be 0 / NULL) */
    uint32_t n_texels;
    const float *texels;        /* n_texels * 3 coefficients, a bitmap's texels row-major, row 0 first */
} msk_scene_desc;

/*
 * Render parameters = the integrator/sampler properties of the reference
 * (integrator.cpp:20-23,130-136; sampler.cpp:8-9) plus the shard selectors.
 * Defaults that reproduce the reference's effective behaviour:
 * rr_depth 5, max_depth -1, hide_emitters 0, block_size 32.
 */
typedef struct msk_render_params {
    uint32_t spp;            /* sampler sample_count; at most 2^20 OWNED samples per pixel and call (the s below; shard more with sample_first / sample_stride) */
    uint64_t seed;           /* sampler base_seed                              */
    int32_t  rng_mode;       /* MSK_RNG_*                                      */
    int32_t  rr_depth;
    int32_t  max_depth;
    int32_t  hide_emitters;
    int32_t  block_size;     /* MSK_BLOCK_SIZE = 32 (imageblock.h:8)           */
    /* shard: this call renders the spiral blocks id with
       id % block_stride == block_first (imageblock.cpp:187-247 order) ...     */
    uint32_t block_first, block_stride;
    /* ... and of every pixel the sample indices s = sample_first + k * sample_stride (k = 0, 1, ...) below spp.
       (0,1) = everything; (r,G) = rank r's interleaved share of G; (a,1) with spp = b = the contiguous range [a, b),
       which lets shares of unequal size be handed out (misaki-render_amd/multigpu.py).
       MSK_RNG_PCG_BLOCK takes (0,1) only (MSK_ERR_UNSUPPORTED otherwise): a block's samples share one sequential PCG32 stream
       (samplers/independent.cpp:9-35), so shards of its sample indices would all draw the same numbers; that mode shards
       by blocks.                                                                                                 */
    uint32_t sample_first, sample_stride;
} msk_render_params;

typedef struct msk_stats {
    uint64_t samples;        /* camera samples traced                          */
    uint64_t segments;       /* closest-hit rays (path segments)               */
    uint64_t shadow_rays;    /* occlusion rays                                 */
    uint32_t iterations;     /* wavefront iterations                           */
    uint32_t passes;         /* block groups (record-buffer passes)            */
    float    ms_total;       /* device time of the whole call                  */
    float    ms_generate;    /* always 0: camera-ray generation is fused into the shading kernel (its time
                                is part of ms_shade); the field keeps the struct layout of ABI v4 */
    /* Sums of the kernel durations of the launches that carried timing events, and how many did
       (n_*_launches).  With the environment variable MSK_TIMING_EVERY=n (default 1) only the launches of
       every n-th group of wavefront iterations are timed: ms_trace / ms_shade are then SAMPLES — divide by
       n_*_launches for an average launch, scale by iterations / n_*_launches for an estimate of the total.
       When the wavefront loop runs on several streams launches overlap, so these sums can
       exceed ms_total.  ms_resolve (film replay + Film::put) is always complete. */
    float    ms_trace, ms_shade, ms_resolve;
    uint32_t n_trace_launches, n_shade_launches;
    /* kernel launches the call actually made (timed or not): traversal kernels, k_shade_gen, k_wavefront (the device-side
       loop of the thin end of a pass, booked as up to 16 `iterations` each) */
    uint32_t launches_trace, launches_shade, launches_wavefront;
    /* ABI v6: samples ImageBlock::put would have warned about (imageblock.cpp:57-81, "Invalid sample value: [...]"): a value of
       the sample's X, Y, Z (or of the nested integrator's R, G, B under "aov") that is not finite, or — "path" only: the
       reference switches the test off for blocks with AOV channels, integrator.cpp:59-60 — below -1e-5.  Such a sample is
       splatted all the same, as the reference does; the plugin logs the count at Warn level. */
    uint64_t invalid_samples;
    /* ABI v7: the bytes of SoA path state the call's launches of the shading / traversal kernels were ASKED to move — counted
       by the library from its own layout (what a live slot makes its kernels read and write), not measured:
       shading 176 B per segment (+ 16 in the general variant) - 64 B per sample + 48 B per shadow ray + 20 B per sample record;
       traversal 48 B per segment + 32 B (16 B for trees in HBM) per shadow ray.  bytes / launches_* = the algorithmic bytes per
       launch a roofline needs; HBM traffic is a separate, measured figure (rocprofv3 PMC).  0 for MSK_RNG_PCG_BLOCK renders. */
    uint64_t bytes_shade, bytes_trace;
} msk_stats;

typedef struct msk_ctx   msk_ctx;
typedef struct msk_scene msk_scene;

/* ---- lifetime ------------------------------------------------------------ */
/* device_ids: n >= 1 HIP ordinals (at most 8).  n == 1: an ordinary context on that device.  n > 1: a GROUP context
   (SURVEY §8b writes the entry point with a device list; csrc/msk_multi.h): one member context per entry — an ordinal may
   repeat —, every scene created on it lives on every member, msk_gpu_render / _render_device / _render_aov shard the call's
   samples over the members by index (member k: sample_first + (k + j n) sample_stride; a MSK_RNG_PCG_BLOCK call, whose
   samples cannot be sharded, by spiral block: block_first + (k + j n) block_stride), one host thread each, and sum the
   films on device_ids[0] over peer access in member order; d_film_xyzaw of msk_gpu_render_device is memory of device_ids[0];
   the sub-stage entry points run on the first member.  msk_stats of a group call: samples / segments / shadow_rays / launches_* and
   the kernel-time samples ms_trace / ms_shade / n_*_launches are SUMS over the members (device time of n devices: not comparable
   with ms_total), iterations / passes / ms_resolve the members' maxima, ms_total the HOST WALL TIME of the whole call (the members'
   renders side by side + the film sum).  (The one-process-per-GPU scheme — one single-device msk_ctx per
   rank + an RCCL film reduce — sits above this ABI: DESIGN.md §7.) */
int  msk_gpu_init(const int *device_ids, int n, msk_ctx **out_ctx);
void msk_gpu_shutdown(msk_ctx *ctx);
const char *msk_gpu_last_error(const msk_ctx *ctx); /* ctx may be NULL */

/* replaces Scene::accel_init (scene.cpp:201-212): upload geometry, build BVH,
   area-light tables (mesh.cpp:39-48).
   Node boxes are padded by 1e-5 (the D10 triangle bounds by 0.5e-5) of the scene's scale = max(diagonal, largest |coordinate|),
   so that the slab test never culls what the triangle test accepts.  Measured margin (tests/test_padding_margin.py,
   test_gpu_trees_equal_brute_force_with_a_tenth_of_the_padding): tree and brute force agree down to 1e-7 of the scale and
   part at 1e-8 — the rule keeps a factor of ~100.  The environment variable MSK_PAD_SCALE (margin tests only; the oracle
   reads it too) replaces the 1e-5; a value that is not a number in [1e-7, 1e-3] fails the call with MSK_ERR_INVALID_ARG. */
int  msk_gpu_scene_create(msk_ctx *ctx, const msk_scene_desc *desc, msk_scene **out_scene);
/* The same with the image of an MSK_EMITTER_ENVMAP emitter; msk_gpu_scene_create(c, d, o) is msk_gpu_scene_create_env(c, d, NULL, o).
   A type-2 emitter without `env`, `env` without a type-2 emitter, a second environment emitter, a zero size, a texel factor or
   weight that is negative or not finite, weights that are all zero and a to_world that is no rotation are MSK_ERR_INVALID_ARG.
   A group context creates the image on every member. */
int  msk_gpu_scene_create_env(msk_ctx *ctx, const msk_scene_desc *desc, const msk_envmap_desc *env, msk_scene **out_scene);
/* The same with everything msk_scene_ext holds; msk_gpu_scene_create_env(c, d, e, o) is msk_gpu_scene_create_ext(c, d, &{e, 0, NULL}, o)
   and ext == NULL is {NULL, 0, NULL}.  MSK_ERR_INVALID_ARG, with a message that names the emitter: an MSK_EMITTER_POINT emitter
   without its msk_point_desc, with two of them, an msk_point_desc whose emitter is of another type (or out of range), a position
   that is not finite, a point emitter whose mesh_id is not -1.  A group context passes the extension to every member. */
int  msk_gpu_scene_create_ext(msk_ctx *ctx, const msk_scene_desc *desc, const msk_scene_ext *ext, msk_scene **out_scene);
/* The same with everything msk_scene_masks holds: msk_gpu_scene_create_ext(c, d, e, o) is msk_gpu_scene_create_masks(c, d, &{*e, 0, NULL}, o)
   and em == NULL is no extension at all.  MSK_ERR_INVALID_ARG, with a message that names the mask: an msk_mask_desc whose bsdf is
   out of range, two of them on one entry, a constant or a value outside [0, 1] or not finite, a filter outside 0..2, an image of
   zero width or height (or without values).  A scene that holds a mask runs kernels of its own (k_shade_gen_m, ...), whatever else
   it holds.  A group context passes the extension to every member. */
int  msk_gpu_scene_create_masks(msk_ctx *ctx, const msk_scene_desc *desc, const msk_scene_masks *em, msk_scene **out_scene);
/* The same with everything msk_scene_lights holds: msk_gpu_scene_create_masks(c, d, m, o) is msk_gpu_scene_create_lights(c, d, &{*m, 0, NULL}, o)
   and el == NULL is no extension at all.  The refusals are listed at msk_light_desc.  A scene that holds a spot or a directional
   emitter runs the kernels of a scene with a point emitter.  A group context passes the extension to every member. */
int  msk_gpu_scene_create_lights(msk_ctx *ctx, const msk_scene_desc *desc, const msk_scene_lights *el, msk_scene **out_scene);
/* The same with everything msk_scene_lens holds: msk_gpu_scene_create_lights(c, d, l, o) is msk_gpu_scene_create_lens(c, d, &{*l, NULL}, o);
   with lens == NULL the call IS msk_gpu_scene_create_lights(c, d, &el->lights, o), and el == NULL is no extension at all.  The
   refusals are listed at msk_lens_desc.  A group context passes the extension to every member. */
int  msk_gpu_scene_create_lens(msk_ctx *ctx, const msk_scene_desc *desc, const msk_scene_lens *el, msk_scene **out_scene);
void msk_gpu_scene_destroy(msk_scene *scene);

/* ---- the hot path --------------------------------------------------------- */
/*
 * Replaces the body of SamplingIntegrator::render between film->prepare() and
 * the last film->put() (integrator.cpp:48-76).  Writes the film's weighted sums
 * {X,Y,Z,A,W} per pixel of the crop window (the whole film by default), row-major
 * crop_height*crop_width*5 floats, exactly what HDRFilm's storage ImageBlock holds
 * after the last put (hdrfilm.cpp:37-38,43-46).
 * film_xyzaw: host memory, caller-owned.  If it is pinned (hipHostMalloc / hipHostRegister) the film is copied into it
 * directly by DMA; a pageable array is filled from the library's own pinned staging buffer.  stats may be NULL.
 */
int  msk_gpu_render(msk_scene *scene, const msk_render_params *params,
                    float *film_xyzaw, msk_stats *stats);

/* Same, but the film stays in HBM: d_film_xyzaw is a device pointer on the
   ctx's device (e.g. a torch tensor's data_ptr, reduced over RCCL afterwards).
   hip_stream: a hipStream_t or NULL for the library's own stream; the call
   returns after the work is complete on that stream. */
int  msk_gpu_render_device(msk_scene *scene, const msk_render_params *params,
                           float *d_film_xyzaw, void *hip_stream, msk_stats *stats);

/*
 * AOVIntegrator::render (integrators/aov.cpp:87-144 through SamplingIntegrator::render, integrator.cpp:31-80):
 * the same job with extra film channels.  aov_types: n_aovs values MSK_AOV_*, in the order of the plugin's
 * m_aov_types; at most one MSK_AOV_PATH_RGBA (the nested "path" integrator whose sample also becomes the
 * XYZ result, aov.cpp:138-139; without one XYZ is 0 — the reference returns an uninitialised Spectrum there).
 * Every AOV value of a camera ray that misses the scene is 0 (the reference reads an uninitialised
 * SceneInteraction for all but depth).  film: crop_height*crop_width*(5 + msk_gpu_aov_channels()) floats, host,
 * the weighted sums HDRFilm's storage holds (channels X,Y,Z,A,W, then the AOV channels in order).
 */
uint32_t msk_gpu_aov_channels(const int32_t *aov_types, uint32_t n_aovs);   /* 0 if a type is invalid */
int  msk_gpu_render_aov(msk_scene *scene, const msk_render_params *params,
                        const int32_t *aov_types, uint32_t n_aovs, float *film, msk_stats *stats);

/* ---- sub-stage entry points (parity tests bind these) ---------------------- */
/*
 * Scene::ray_intersect / Scene::ray_test (scene.cpp:216-273) on a batch of
 * rays.  rays: n * 8 floats {ox,oy,oz,tmin, dx,dy,dz,tmax}.
 * closest: out_hit n * 4 floats {t,u,v, bitcast(prim)} with t = +inf on a
 * miss; prim is the scene-global triangle index (mesh.first_face + primID).
 * any: out_occluded n bytes (0/1).  Host pointers.
 */
int  msk_gpu_trace_closest(msk_scene *scene, uint64_t n, const float *rays, float *out_hit);
int  msk_gpu_trace_any(msk_scene *scene, uint64_t n, const float *rays, uint8_t *out_occluded);

/*
 * render_sample (integrator.cpp:103-126) for every sample of the listed
 * pixels, WITHOUT the film splat: out_xyz = n_pixels * spp * 3 floats, the
 * {X,Y,Z} that render_sample hands to ImageBlock::put, out_pos (may be NULL)
 * = n_pixels * spp * 2 floats position_sample.  pixels: n_pixels * 2 int32
 * (x,y).  counter RNG only.  Host pointers.
 */
int  msk_gpu_sample_pixels(msk_scene *scene, const msk_render_params *params,
                           uint64_t n_pixels, const int32_t *pixels,
                           float *out_xyz, float *out_pos);

/*
 * The camera ray of n film positions: film_pos n * 2 floats (px, py) in pixels, aperture_u n * 2 floats in [0, 1) (the aperture
 * sample; read only by a scene with a lens, may be NULL otherwise); out_rays n * 8 floats {o.x, o.y, o.z, tnear, d.x, d.y, d.z, tfar},
 * the layout msk_gpu_trace_closest reads.  The kernel calls the one device function the render kernels call, for the pinhole as for
 * the lens (msk_lens_desc).  Host pointers.  A group context runs it on its first member.
 */
int  msk_gpu_camera_sample(msk_scene *scene, uint64_t n, const float *film_pos, const float *aperture_u, float *out_rays);

/*
 * A texture's value at n surface points (SmoothDiffuse::m_reflectance->eval(si) for given si.uv): uv n * 2 floats,
 * wavelengths n * 4, out n * 4 floats; texture is 1-based, as msk_bsdf_desc::reflectance_texture.  The kernel calls the
 * device function the shading kernels call, for checkerboards as for bitmaps.  Host pointers.  ABI v8.
 */
int  msk_gpu_eval_texture(msk_scene *scene, uint32_t texture, uint64_t n, const float *uv, const float *wavelengths, float *out);

/*
 * The environment image at n directions (unit vectors): dirs n * 3, wavelengths n * 4;
 * out_radiance n * 4 = L(direction, l), out_pdf n = pdf_omega(direction) (without the 1 / n_emitters of light selection).
 * msk_gpu_env_sample: u n * 2 -> the direction, uv and pdf_omega the next-event branch draws.  Both run the device functions the
 * shading kernels call.  Host pointers; MSK_ERR_INVALID_ARG for a scene without an MSK_EMITTER_ENVMAP emitter.
 */
int  msk_gpu_env_eval(msk_scene *scene, uint64_t n, const float *dirs, const float *wavelengths, float *out_radiance, float *out_pdf);
int  msk_gpu_env_sample(msk_scene *scene, uint64_t n, const float *u, float *out_dir, float *out_uv, float *out_pdf);

/*
 * The next-event sample of point emitter `emitter` (index into `emitters`) from n reference points: ref_points n * 3,
 * wavelengths n * 4; out_d_dist n * 4 = {d.x, d.y, d.z, dist}, out_value n * 4 = value(l) (without the light-selection factor);
 * all zeros where dist == 0.  msk_gpu_conductor_sample: the lobe's value of BSDF `bsdf` (index into `bsdfs`) for n cos_theta_i:
 * out_value n * 4, zeros for cos_i <= 0.  Both run the device functions the shading kernels call.  Host pointers;
 * MSK_ERR_INVALID_ARG for an index that is out of range or of another type.
 */
int  msk_gpu_point_sample(msk_scene *scene, uint32_t emitter, uint64_t n, const float *ref_points, const float *wavelengths, float *out_d_dist, float *out_value);
int  msk_gpu_conductor_sample(msk_scene *scene, uint32_t bsdf, uint64_t n, const float *cos_theta_i, const float *wavelengths, float *out_value);
/*
 * The next-event sample of the spot or directional emitter `emitter` (msk_light_desc), with the arguments and outputs of
 * msk_gpu_point_sample, through the device function the shading kernels call.  A spot: {d, dist} and value(l) = ((I inv) inv) f, the
 * value all zeros where f == 0, everything zeros where dist == 0.  A sun: {-direction, 2 env_radius} and E(l), whatever the
 * reference point.  MSK_ERR_INVALID_ARG for an emitter that is out of range or neither a spot nor a directional emitter.
 */
int  msk_gpu_light_sample(msk_scene *scene, uint32_t emitter, uint64_t n, const float *ref_points, const float *wavelengths, float *out_d_dist, float *out_value);

/*
 * The decorated BSDF entry `bsdf` of a scene that holds a mask (msk_mask_desc; an entry without one has the constant opacity 1), at n
 * points, through the device functions the shading kernels call.  uv n * 2, wi n * 3 (local frame, either face), wavelengths n * 4.
 * msk_gpu_mask_sample: sample1_u n * 3 = {sample1, u.x, u.y}; out_wo_pdf n * 4 = {wo.x, wo.y, wo.z, pdf} (the null lobe: wo = -wi,
 * the local form of "the ray's own direction"), out_value n * 4, out_flags n * 4 = {eta, delta (1 / 0), null lobe (1 / 0), a
 * direction was produced (1 / 0)}.  msk_gpu_mask_eval: wo n * 3; out_a_pdf n * 2 = {a, pdf}, out_value n * 4 = eval.
 * Host pointers; MSK_ERR_INVALID_ARG for a scene without a mask or an entry out of range.
 */
int  msk_gpu_mask_sample(msk_scene *scene, uint32_t bsdf, uint64_t n, const float *uv, const float *wi, const float *sample1_u, const float *wavelengths,
                         float *out_wo_pdf, float *out_value, float *out_flags);
int  msk_gpu_mask_eval(msk_scene *scene, uint32_t bsdf, uint64_t n, const float *uv, const float *wi, const float *wo, const float *wavelengths,
                       float *out_a_pdf, float *out_value);

/*
 * The same two probes on a MSK_BSDF_PLASTIC entry, in a scene with or without a mask (without one every entry has the constant opacity
 * 1): arguments and outputs as msk_gpu_mask_sample / msk_gpu_mask_eval.  out_flags n * 4 = {eta, the sampled lobe was delta (1 / 0:
 * the coat, or a mask's null lobe), null lobe (1 / 0), a direction was produced (1 / 0)}.  MSK_ERR_INVALID_ARG for an entry out of
 * range or one that is not a plastic.
 * msk_gpu_plastic_constants: out = {fdr_int, ssw}, the two constants the packer computed for the entry (msk_bsdf_desc), as the
 * kernels read them.  No device work.
 */
int  msk_gpu_plastic_sample(msk_scene *scene, uint32_t bsdf, uint64_t n, const float *uv, const float *wi, const float *sample1_u, const float *wavelengths,
                            float *out_wo_pdf, float *out_value, float *out_flags);
int  msk_gpu_plastic_eval(msk_scene *scene, uint32_t bsdf, uint64_t n, const float *uv, const float *wi, const float *wo, const float *wavelengths,
                          float *out_a_pdf, float *out_value);
int  msk_gpu_plastic_constants(msk_scene *scene, uint32_t bsdf, float out[2]);
/*
 * The two probes on a MSK_BSDF_ROUGHPLASTIC entry: arguments and outputs as msk_gpu_plastic_sample / msk_gpu_plastic_eval (the delta
 * flag is 0 unless a mask's null lobe was sampled).  MSK_ERR_INVALID_ARG for an entry out of range or one that is not a roughplastic.
 * msk_gpu_plastic_constants answers for a roughplastic entry too.
 */
int  msk_gpu_roughplastic_sample(msk_scene *scene, uint32_t bsdf, uint64_t n, const float *uv, const float *wi, const float *sample1_u, const float *wavelengths,
                                 float *out_wo_pdf, float *out_value, float *out_flags);
int  msk_gpu_roughplastic_eval(msk_scene *scene, uint32_t bsdf, uint64_t n, const float *uv, const float *wi, const float *wo, const float *wavelengths,
                               float *out_a_pdf, float *out_value);

/* ---- the "direct" integrator ----------------------------------------------- */
/*
 * Direct illumination only (integrators/direct.cpp): per camera sample one primary ray, `light_samples` next-event samples and
 * `bsdf_samples` BSDF samples at the primary hit, combined by the power heuristic over the sample COUNTS:
 *   w_l = (N p_l)^2 / ((N p_l)^2 + (M p_b)^2),  w_b = (M p_b)^2 / ((M p_b)^2 + (N p_e)^2),  terms divided by N and M.
 * Random pairs of a sample (counter_pair of its key): 0-2 as "path" (film position, wavelengths, aperture), 3 + i light sample i,
 * 3 + N + 2 j / + 1 the lobe choice (.x) and the direction of BSDF sample j; additions in the order emission, light samples,
 * BSDF samples.  The fp32 operations of a term, in order (each its own rounded operation, per wavelength; N and M as floats):
 *   weight(n_a, p_a, n_b, p_b):  a = n_a * p_a;  b = n_b * p_b;  a = a * a;  b = b * b;  a > 0 ? a / (a + b) : 0
 *   light sample i:  t = emitter_val * bsdf_val;  t = t * w_l;  w_l = weight(N, p_l, M, p_b), or 1 for a point light;
 *                    a shadow ray is traced (and counted) iff t is not zero at every wavelength; unoccluded: t = t / N; result += t
 *   BSDF sample j:   traced (and counted as a segment) iff the sample succeeded and bsdf_val is not zero at every wavelength;
 *                    reaching an emitter or an environment:  t = bsdf_val * value;  t = t * w_b;  w_b = weight(M, p_b, N, p_e);
 *                    t = t / M;  result += t
 * p_l and p_e carry the light-selection factor 1 / n_emitters; emitter_val is the radiance over p_l (a point light: I / d^2 times
 * n_emitters).  With (1, 1) the result is, bit for bit, msk_gpu_render at max_depth = 2 — except for a `constant` sky in a scene
 * of the older kernel families, which counts here with the density of the ray's own direction always.
 * light_samples and bsdf_samples are each in [0, 4096] and not both 0 (MSK_ERR_INVALID_ARG otherwise).
 * msk_render_params: rr_depth and max_depth are ignored; spp, seed, hide_emitters, block_size and the shard selectors mean what
 * they mean for msk_gpu_render.  MSK_RNG_PCG_BLOCK and group contexts: MSK_ERR_UNSUPPORTED (shard over processes with
 * sample_first / sample_stride).  msk_stats: samples, segments, shadow_rays, invalid_samples, passes, ms_total, ms_resolve;
 * iterations = kernel launches of k_direct; the wavefront-only fields are 0.
 * msk_gpu_sample_pixels_direct: msk_gpu_sample_pixels for this integrator; unlike it, it HONOURS sample_first / sample_stride:
 * out_xyz / out_pos hold, per listed pixel, the call's owned samples s = sample_first + k * sample_stride < spp, in order.
 */
typedef struct msk_direct_params { uint32_t light_samples, bsdf_samples; } msk_direct_params;
int  msk_gpu_render_direct(msk_scene *scene, const msk_render_params *params, const msk_direct_params *direct,
                           float *film_xyzaw, msk_stats *stats);
int  msk_gpu_render_direct_device(msk_scene *scene, const msk_render_params *params, const msk_direct_params *direct,
                                  float *d_film_xyzaw, void *hip_stream, msk_stats *stats);
int  msk_gpu_sample_pixels_direct(msk_scene *scene, const msk_render_params *params, const msk_direct_params *direct,
                                  uint64_t n_pixels, const int32_t *pixels, float *out_xyz, float *out_pos);

/* device + build information for logs: fills a NUL-terminated string */
int  msk_gpu_describe(const msk_ctx *ctx, char *buf, uint64_t buf_size);

#ifdef __cplusplus
}
#endif
#endif /* MSK_GPU_H */
