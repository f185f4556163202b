"""The smooth `plastic` BSDF (include/msk_gpu.h at MSK_BSDF_PLASTIC) restated twice, sharing nothing with the code under test.

fp32 side (fresnel32, lobes32, sample32, eval32): numpy float32, one IEEE operation per line, in the order the header gives.  What
varies with the wavelength (rho, s) and the cosine-hemisphere direction come in as arrays: the tests take them from the oracle
binding (srgb_model_eval, warps), which return the device functions' bits.

float64 side: the same BSDF from the textbook (dielectric_ref.fresnel_textbook), the two packer constants (fdr_int by the
identity and by a direct quadrature of another shape; ssw from the means of the spectra), the albedo, and the closed forms of the
render tests.
"""
import numpy as np

import dielectric_ref as DR
import radiometry_ref as R

F = np.float32
INV_PI = F(0.31830988618379067154)
LAMBDAS = 360.0 + 5.0 * np.arange(95)


# ----------------------------------------------------------------------------- fp32
def fresnel32(cos_i, eta):
    """msk_device.h fresnel_dielectric for cos_i >= 0 (the only side a plastic evaluates it on) -> F, float32"""
    c = np.asarray(cos_i, F)
    eta = F(eta)
    eta_ti = F(F(1) / eta)
    with np.errstate(invalid="ignore", divide="ignore"):
        t0 = (eta_ti * eta_ti).astype(F)
        t1 = (F(1) - (c * c).astype(F)).astype(F)
        ct2 = (F(1) - (t0 * t1).astype(F)).astype(F)
        ci = np.abs(c)
        ct = np.sqrt(np.maximum(ct2, F(0))).astype(F)
        a_s = (((ci - (eta * ct).astype(F)).astype(F)) / ((ci + (eta * ct).astype(F)).astype(F))).astype(F)
        a_p = (((ct - (eta * ci).astype(F)).astype(F)) / ((ct + (eta * ci).astype(F)).astype(F))).astype(F)
        r = (F(0.5) * ((a_s * a_s).astype(F) + (a_p * a_p).astype(F)).astype(F)).astype(F)
    if eta == F(1):
        return np.zeros_like(c)
    return np.where(ci == 0, F(1), r).astype(F)


def lobes32(cos_i, eta, ssw):
    """-> (ok, F_i, ps, pd): ps = F_i ssw, pd = (1 - F_i)(1 - ssw), normalised; ok false where cos_i <= 0 or ps + pd == 0"""
    c = np.asarray(cos_i, F)
    ssw = F(ssw)
    f_i = fresnel32(np.maximum(c, F(0)), eta)
    a = (f_i * ssw).astype(F)
    d = ((F(1) - f_i).astype(F) * F(F(1) - ssw)).astype(F)
    s = (a + d).astype(F)
    ok = (c > 0) & (s != 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        ps = (a / s).astype(F)
    pd = (F(1) - ps).astype(F)
    return ok, f_i, ps, pd


def diffuse32(rho, f_i, cos_o, eta, inv_eta, fdr_int, nonlinear):
    """D(l) f with f = inv_eta^2 (1 - F_i)(1 - F_o), products left to right: rho float32 [n, 4] -> float32 [n, 4]"""
    rho, fdr, inv_eta = np.asarray(rho, F), F(fdr_int), F(inv_eta)
    f_o = fresnel32(np.maximum(np.asarray(cos_o, F), F(0)), eta)
    with np.errstate(invalid="ignore", divide="ignore"):
        if nonlinear:
            d = (rho / (F(1) - (fdr * rho).astype(F)).astype(F)).astype(F)
        else:
            d = (rho / F(F(1) - fdr)).astype(F)
    f = ((F(inv_eta * inv_eta) * (F(1) - f_i).astype(F)).astype(F) * (F(1) - f_o).astype(F)).astype(F)
    return (d * f[:, None]).astype(F)


def eval32(wi, wo, rho, eta, inv_eta, fdr_int, ssw, nonlinear):
    """-> (eval float32 [n, 4], pdf float32 [n]): the diffuse lobe alone, for cos_i > 0 and cos_o > 0"""
    wi, wo = np.asarray(wi, F), np.asarray(wo, F)
    ok, f_i, ps, pd = lobes32(wi[:, 2], eta, ssw)
    ok = ok & (wo[:, 2] > 0)
    co = wo[:, 2]
    val = ((diffuse32(rho, f_i, co, eta, inv_eta, fdr_int, nonlinear) * INV_PI).astype(F) * co[:, None]).astype(F)
    pdf = (pd * (INV_PI * co).astype(F)).astype(F)
    return np.where(ok[:, None], val, F(0)).astype(F), np.where(ok, pdf, F(0)).astype(F)


def sample32(wi, sample1, hemi, rho, s, eta, inv_eta, fdr_int, ssw, nonlinear):
    """hemi float32 [n, 3] = square_to_cosine_hemisphere(u); rho, s float32 [n, 4] -> dict(wo, pdf, value, delta, ok); eta is 1"""
    wi, hemi, s1 = np.asarray(wi, F), np.asarray(hemi, F), np.asarray(sample1, F)
    ok, f_i, ps, pd = lobes32(wi[:, 2], eta, ssw)
    coat = ok & (s1 < ps)
    base = ok & ~coat
    n = len(wi)
    wo, pdf, val = np.zeros((n, 3), F), np.zeros(n, F), np.zeros((n, 4), F)
    with np.errstate(invalid="ignore", divide="ignore"):
        wo[coat] = np.stack([-wi[coat, 0], -wi[coat, 1], wi[coat, 2]], -1)
        pdf[coat] = ps[coat]
        val[coat] = ((np.asarray(s, F)[coat] * f_i[coat, None]).astype(F) / ps[coat, None]).astype(F)
        wo[base] = hemi[base]
        p = (pd * (INV_PI * hemi[:, 2]).astype(F)).astype(F)
        pdf[base] = p[base]
        v = (diffuse32(rho, f_i, hemi[:, 2], eta, inv_eta, fdr_int, nonlinear) / pd[:, None]).astype(F)
        val[base] = np.where((p > 0)[:, None], v, F(0))[base]
    return dict(wo=wo, pdf=pdf, value=val, delta=coat, ok=ok)


# ----------------------------------------------------------------------------- float64: the constants
def fresnel64(mu, eta):
    """the exact unpolarised reflectance of the boundary seen from the thin side at cos(theta) = mu (textbook form)"""
    return DR.fresnel_textbook(np.arccos(np.clip(mu, 0.0, 1.0)), 1.0, float(eta))


def fdr_ext64(eta, m=64, panels=8):
    total = 0.0
    for k in range(panels):
        mu, w = R.gauss_legendre(m, k / panels, (k + 1) / panels)
        total += float((w * fresnel64(mu, eta) * mu).sum())
    return 2.0 * total


def fdr_int64(eta):
    """the identity: 1 - (1 - fdr_ext) / eta^2"""
    if eta == 1.0:
        return 0.0
    return 1.0 - (1.0 - fdr_ext64(eta)) / (eta * eta)


def fdr_int_direct64(eta, m=64):
    """2 int_0^1 F(mu; 1 / eta) mu dmu from the inside, directly: below the critical cosine mu_c = sqrt(1 - 1 / eta^2) the reflection is
    total (the integral of 2 mu is mu_c^2); above it the integrand has a square-root kink at mu_c, which the substitution
    mu = sqrt(mu_c^2 + t^2 / eta^2), with t = the cosine on the OUTSIDE in [0, 1], takes away (2 mu dmu = 2 t dt / eta^2): another rule than
    the identity's, on another variable"""
    if eta == 1.0:
        return 0.0
    mu_c2 = 1.0 - 1.0 / (eta * eta)
    total = 0.0
    for k in range(8):
        t, w = R.gauss_legendre(m, k / 8.0, (k + 1) / 8.0)
        mu = np.sqrt(mu_c2 + t * t / (eta * eta))
        theta = np.arccos(np.clip(mu, 0.0, 1.0))
        total += float((w * DR.fresnel_textbook(theta, float(eta), 1.0) * 2.0 * t / (eta * eta)).sum())
    return mu_c2 + total


def sigmoid64(coeff, lam):
    c0, c1, c2 = (float(c) for c in coeff)
    lam = np.asarray(lam, np.float64)
    if np.isinf(c2):
        return np.full_like(lam, 1.0 if c2 > 0 else 0.0)
    x = (c0 * lam + c1) * lam + c2
    return np.maximum(0.5 + x / (2.0 * np.sqrt(1.0 + x * x)), 0.0)


def ssw64(s_mean, d_mean):
    return s_mean / (d_mean + s_mean) if (d_mean + s_mean) > 0 else 1.0


def desc_ssw64(desc, b, texels=None):
    """ssw of BSDF entry b of a scene descriptor: the means over the 95 CIE wavelengths of s and of rho (a checkerboard: its two
    colours; a bitmap: its texels, coefficients float32 [n, 3] in `texels`)"""
    bd = desc.bsdfs[b]
    assert bd.specular_reflectance.regular == 0 and bd.reflectance_regular == 0
    s_mean = float(bd.specular_reflectance.scale) * sigmoid64(bd.specular_reflectance.coeff[:], LAMBDAS).mean()
    if bd.reflectance_texture == 0:
        d_mean = float(bd.reflectance_scale) * sigmoid64(bd.reflectance[:], LAMBDAS).mean()
    else:
        td = desc.textures[bd.reflectance_texture - 1]
        if td.type == 1:
            d_mean = 0.5 * (sigmoid64(td.color0[:], LAMBDAS).mean() + sigmoid64(td.color1[:], LAMBDAS).mean())
        else:
            tx = np.asarray(texels, np.float64).reshape(-1, 3)[td.first_texel:td.first_texel + td.width * td.height]
            d_mean = float(np.mean([sigmoid64(c, LAMBDAS).mean() for c in tx]))
    return ssw64(s_mean, d_mean)


# ----------------------------------------------------------------------------- float64: the BSDF and its albedo
def base64(rho, eta, nonlinear):
    fdr = fdr_int64(eta)
    return rho / (1.0 - fdr * rho) if nonlinear else rho / (1.0 - fdr)


def eval64(cos_i, cos_o, rho, eta, nonlinear):
    """the diffuse lobe's value with its cosine: D / eta^2 (1 - F_i)(1 - F_o) cos_o / pi"""
    return base64(rho, eta, nonlinear) / (eta * eta) * (1.0 - fresnel64(cos_i, eta)) * (1.0 - fresnel64(cos_o, eta)) * cos_o / np.pi


def albedo64(cos_i, rho, s, eta, nonlinear):
    """F_i s + (1 - F_i) D (1 - fdr_int): the integral of the diffuse lobe over the hemisphere, int (1 - F_o) cos_o / pi = 1 - fdr_ext =
    eta^2 (1 - fdr_int), plus the coat"""
    f_i = fresnel64(cos_i, eta)
    return f_i * s + (1.0 - f_i) * base64(rho, eta, nonlinear) * (1.0 - fdr_int64(eta))


def estimator_mean64(cos_i, rho, s, eta, ssw, nonlinear, m=64):
    """E[value] of sample() by quadrature: the coat's branch has mass ps and value s F_i / ps; the diffuse branch mass pd and value
    D f / pd over the cosine-weighted hemisphere"""
    f_i = float(fresnel64(cos_i, eta))
    ps, pd = f_i * ssw, (1.0 - f_i) * (1.0 - ssw)
    if ps + pd == 0:
        return 0.0
    ps = ps / (ps + pd)
    pd = 1.0 - ps
    total = ps * (s * f_i / ps) if ps > 0 else 0.0
    if pd > 0:
        for k in range(8):
            z, w = R.gauss_legendre(m, k / 8.0, (k + 1) / 8.0)        # the density of z = wo.z is 2 z
            val = base64(rho, eta, nonlinear) / (eta * eta) * (1.0 - f_i) * (1.0 - fresnel64(z, eta)) / pd
            total += pd * float((w * 2.0 * z * val).sum())
    return total
