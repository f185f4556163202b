// msk_plastic_tables.h — the `plastic` part of msk_scene_tables.h (include/msk_gpu.h: MSK_BSDF_PLASTIC): the refusals of a type-6
// descriptor, the two constants the packer computes per entry, and what a scene with a plastic needs of the tables.  Plain C++17, no
// HIP; tests/native/plastic_tables_check.cpp checks every refusal and both constants on a CPU.
// A type-6 entry's device record is the 7-float4 BSDF record of every type; the two constants stand in the words the type leaves
// unused, where alpha_u and alpha_v stand for the rough types: word 5 = fdr_int, word 6 = ssw (msk_kernels.h: plastic_sample).
// A scene with a plastic runs the SceneTablesM instantiations, which carry the mask code: such a scene must have the mask records at the
// end of `bsdfs`.  One that holds no mask gets them here, every entry the constant opacity 1, as a scene with a lens does
// (msk_lens_tables.h).
// A type-7 entry (MSK_BSDF_ROUGHPLASTIC) keeps alpha where the rough types keep alpha_u (word 5; word 6 = alpha_v, equal to it) and
// `nonlinear` where type 6 keeps it (word 7); its two constants stand in the first two words of the specular_transmittance float4,
// which the type does not read: word 20 = fdr_int, word 21 = ssw (msk_kernels.h: roughplastic_sample).  It sets has_plastic too.
#pragma once
#include "../../include/msk_gpu.h"

#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

namespace mskscene {

// the text of a refusal, as msk_gpu.hip's fail_to writes it
inline int refuse_plastic(std::string *msg, int code, const char *fmt, ...) {
    char buf[1024];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
    *msg = buf;
    return code;
}

// the words of the 28-float BSDF record that hold {fdr_int, ssw} (ssw follows fdr_int)
constexpr uint32_t kPlasticConstantsWord = 5, kRoughPlasticConstantsWord = 20;
inline uint32_t plastic_constants_word(int32_t type) { return type == MSK_BSDF_ROUGHPLASTIC ? kRoughPlasticConstantsWord : kPlasticConstantsWord; }

// what pack_bsdfs asks of a type-6 descriptor beyond what it asks of every type (who: the type's name in the text)
inline int check_plastic(const msk_bsdf_desc &bd, uint32_t b, std::string *msg, const char *who = "plastic") {
    if (!(std::isfinite(bd.ior_eta) && bd.ior_eta >= 1.f))
        return refuse_plastic(msg, MSK_ERR_INVALID_ARG, "bsdf %u: %s: the relative index of refraction ior_eta %g must be finite and at least 1 "
                              "(int_ior / ext_ior of a coat denser than what surrounds it)", b, who, (double) bd.ior_eta);
    if (!(std::isfinite(bd.ior_inv_eta) && bd.ior_inv_eta > 0.f))
        return refuse_plastic(msg, MSK_ERR_INVALID_ARG, "bsdf %u: %s: ior_inv_eta %g must be finite and positive", b, who, (double) bd.ior_inv_eta);
    if (bd.specular_reflectance.regular == 0 && !std::isfinite(bd.specular_reflectance.scale))
        return refuse_plastic(msg, MSK_ERR_INVALID_ARG, "bsdf %u: %s: the scale of specular_reflectance must be finite", b, who);
    return MSK_OK;
}
// ... and of a type-7 one: type 6's checks, and one finite, non-negative roughness (roughplastic.cpp:23-25 refuses an anisotropic coat)
inline int check_roughplastic(const msk_bsdf_desc &bd, uint32_t b, std::string *msg) {
    if (int rc = check_plastic(bd, b, msg, "roughplastic")) return rc;
    if (!(std::isfinite(bd.alpha_u) && std::isfinite(bd.alpha_v) && bd.alpha_u >= 0.f && bd.alpha_v >= 0.f))
        return refuse_plastic(msg, MSK_ERR_INVALID_ARG, "bsdf %u: roughplastic: the roughness alpha (%g, %g) must be finite and non-negative", b,
                              (double) bd.alpha_u, (double) bd.alpha_v);
    if (bd.alpha_u != bd.alpha_v)
        return refuse_plastic(msg, MSK_ERR_INVALID_ARG, "bsdf %u: roughplastic: alpha_u %g and alpha_v %g differ: anisotropic coats are not supported", b,
                              (double) bd.alpha_u, (double) bd.alpha_v);
    return MSK_OK;
}

// render/fresnel.h:37-63 in double, for cos_theta_i >= 0: the exact unpolarised reflectance of a smooth dielectric boundary
inline double plastic_fresnel(double cos_i, double eta) {
    if (eta == 1.0) return 0.0;
    if (cos_i <= 0.0) return 1.0;
    const double inv = 1.0 / eta;
    const double ct2 = 1.0 - inv * inv * (1.0 - cos_i * cos_i);
    const double ct = std::sqrt(ct2 > 0.0 ? ct2 : 0.0);
    const double a_s = (cos_i - eta * ct) / (cos_i + eta * ct), a_p = (ct - eta * cos_i) / (ct + eta * cos_i);
    return 0.5 * (a_s * a_s + a_p * a_p);
}

// fdr_ext = 2 int_0^1 F(mu; eta) mu dmu by a 64-point Gauss-Legendre rule on each of four equal panels (the integrand is smooth for
// eta >= 1; the nodes by Newton's iteration on P_64), then fdr_int = 1 - (1 - fdr_ext) / eta^2 (exact: msk_gpu.h)
inline double plastic_fdr_int(double eta) {
    constexpr int N = 64, PANELS = 4;
    static double xs[N], ws[N];
    static bool have = false;
    if (!have) {
        const double pi = 3.14159265358979323846;
        for (int i = 0; i < N; ++i) {
            double x = std::cos(pi * (i + 0.75) / (N + 0.5)), dp = 1.0;
            for (int it = 0; it < 100; ++it) {
                double p0 = 1.0, p1 = x;
                for (int k = 2; k <= N; ++k) { const double p2 = ((2.0 * k - 1.0) * x * p1 - (k - 1.0) * p0) / k; p0 = p1; p1 = p2; }
                dp = N * (x * p1 - p0) / (x * x - 1.0);
                const double dx = p1 / dp;
                x -= dx;
                if (std::fabs(dx) < 1e-16) break;
            }
            {   // the derivative at the converged node
                double p0 = 1.0, p1 = x;
                for (int k = 2; k <= N; ++k) { const double p2 = ((2.0 * k - 1.0) * x * p1 - (k - 1.0) * p0) / k; p0 = p1; p1 = p2; }
                dp = N * (x * p1 - p0) / (x * x - 1.0);
            }
            xs[i] = x; ws[i] = 2.0 / ((1.0 - x * x) * dp * dp);
        }
        have = true;
    }
    double sum = 0.0;
    for (int p = 0; p < PANELS; ++p) {
        const double a = (double) p / PANELS, h = 1.0 / PANELS;
        for (int i = 0; i < N; ++i) {
            const double mu = a + 0.5 * h * (xs[i] + 1.0);
            sum += 0.5 * h * ws[i] * plastic_fresnel(mu, eta) * mu;
        }
    }
    const double fdr_ext = 2.0 * sum;
    return 1.0 - (1.0 - fdr_ext) / (eta * eta);
}

// render/srgb.h:8-19 in double: the sigmoid polynomial S(c, l)
inline double plastic_srgb(const float *c, double l) {
    if (std::isinf(c[2])) return c[2] > 0.f ? 1.0 : 0.0;
    const double v = ((double) c[0] * l + (double) c[1]) * l + (double) c[2];
    const double r = 0.5 * v / std::sqrt(v * v + 1.0) + 0.5;
    return r > 0.0 ? r : 0.0;
}
// the mean of scale * S(c, l) over the 95 CIE sample wavelengths, 360 nm to 830 nm in steps of 5
inline double plastic_mean_srgb(const float *c, double scale) {
    double s = 0.0;
    for (int i = 0; i < MSK_CIE_SAMPLES; ++i) s += plastic_srgb(c, 360.0 + 5.0 * i);
    return scale * s / MSK_CIE_SAMPLES;
}
// ... of the tabulated spectrum regular_spectra[k - 1] (msk_regular_spectrum_desc: lerp, the end segments continued)
inline double plastic_mean_regular(const msk_scene_desc *d, uint32_t k) {
    const msk_regular_spectrum_desc &r = d->regular_spectra[k - 1];
    const double inv = 1.0 / (((double) r.lambda_max - (double) r.lambda_min) / (double) (r.size - 1));
    double s = 0.0;
    for (int i = 0; i < MSK_CIE_SAMPLES; ++i) {
        const double x = (360.0 + 5.0 * i - (double) r.lambda_min) * inv;
        long idx = x > 0.0 ? (long) x : 0;
        if (idx > (long) r.size - 2) idx = (long) r.size - 2;
        const double w1 = x - (double) idx;
        s += (1.0 - w1) * d->regular_values[r.first_value + idx] + w1 * d->regular_values[r.first_value + idx + 1];
    }
    return s / MSK_CIE_SAMPLES;
}
inline double plastic_mean_spectrum(const msk_scene_desc *d, const msk_spectrum_desc &sp) {
    return sp.regular ? plastic_mean_regular(d, sp.regular) : plastic_mean_srgb(sp.coeff, (double) sp.scale);
}
// the mean of the diffuse reflectance of entry bd, as MSK_BSDF_DIFFUSE reads it.  The descriptor has passed pack_textures / pack_bsdfs
inline double plastic_mean_reflectance(const msk_scene_desc *d, const msk_bsdf_desc &bd) {
    if (bd.reflectance_regular) return plastic_mean_regular(d, bd.reflectance_regular);
    if (!bd.reflectance_texture) return plastic_mean_srgb(bd.reflectance, (double) bd.reflectance_scale);
    const msk_texture_desc &td = d->textures[bd.reflectance_texture - 1];
    if (td.type == MSK_TEXTURE_CHECKERBOARD) return 0.5 * (plastic_mean_srgb(td.color0, 1.0) + plastic_mean_srgb(td.color1, 1.0));
    const size_t n = (size_t) td.width * td.height;
    double s = 0.0;
    for (size_t k = 0; k < n; ++k) s += plastic_mean_srgb(d->texels + ((size_t) td.first_texel + k) * 3, 1.0);
    return s / (double) n;
}

// {fdr_int, ssw} of a type-6 or type-7 entry, rounded to fp32
inline void plastic_constants(const msk_scene_desc *d, const msk_bsdf_desc &bd, float out[2]) {
    out[0] = (float) plastic_fdr_int((double) bd.ior_eta);
    const double s_mean = plastic_mean_spectrum(d, bd.specular_reflectance), d_mean = plastic_mean_reflectance(d, bd);
    out[1] = (d_mean + s_mean) > 0.0 ? (float) (s_mean / (d_mean + s_mean)) : 1.f;
}

// mask records of the constant opacity 1 for every entry of a scene that has none of its own: the record pack_mask_records
// (msk_mask_tables.h) writes for an entry without a mask, under which the mask code is the nested BSDF to the bit
inline void add_unit_mask_records(uint32_t n_bsdfs, std::vector<float> &bsdfs, uint32_t &n_bsdf_f4, uint32_t &mask_base) {
    mask_base = n_bsdf_f4;
    n_bsdf_f4 += 3u * n_bsdfs;
    bsdfs.resize((size_t) n_bsdf_f4 * 4, 0.f);
    for (uint32_t b = 0; b < n_bsdfs; ++b) bsdfs[((size_t) mask_base + 3u * b + 1u) * 4 + 1] = 1.f;      // {filter 0 = constant, opacity 1}
}

}  // namespace mskscene
