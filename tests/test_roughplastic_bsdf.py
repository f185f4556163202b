"""The `roughplastic` BSDF (include/msk_gpu.h at MSK_BSDF_ROUGHPLASTIC): the plastic with a GGX coat, two smooth lobes, in the mask family.

The device is held in three ways: to the fp32 restatement (roughplastic_ref.py) bit for bit through the probes; to float64
expectations through renders; and to itself across every execution variant, under an opacity-1 mask and across sample shards.

CPU: the contract is unbiased in float64 and the reference's `sample_visible = true` density is not (the header's departure); the
packer, its refusals and the plan as a stand-alone native program (also under AddressSanitizer / UBSan); the two flatteners;
exports and struct layouts; the expectations' own convergence.
GPU: probes; expectations (counter RNG through msk_gpu_sample_pixels, and (a), (b) once more through a 32 x 32 film under
MSK_RNG_PCG_BLOCK); identities; an "aov" render; refusals."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import delta_ref as D
import plastic_ref as P
import radiometry_ref as R
import roughplastic_ref as RP
import test_delta_light_mirror as DM
import test_envmap as EV
import test_launch_plan as LP
import test_plastic_bsdf as TP
import test_spot_directional as SD
import test_table_placement as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
CAM, W48, CROP = EV.PLANE_CAMERA, EV.W48, EV.CROP
STEEP, GRAZING, SKY, bits, quad = TP.STEEP, TP.GRAZING, TP.SKY, TP.bits, TP.quad
ONE_BELOW = F(1) - F(2.0 ** -24)


def roughplastic(rho=0.5, s=1.0, eta=1.4896, nonlinear=False, alpha=0.3, **kw):
    return dict({"type": "roughplastic", "diffuse_reflectance": rho, "specular_reflectance": s, "int_ior": eta, "ext_ior": 1.0, "nonlinear": nonlinear,
                 "alpha": alpha}, **kw)


# ===================================================================================================== CPU 1, 2: the contract in float64
# (cos_i, alpha, ior): a grazing view at two roughnesses, a near-mirror coat seen steeply, the roughest coat at a middle view; rho = 0.5, s = 1
POINTS = [(0.1, 0.3, 1.5), (0.9, 0.05, 1.5), (0.5, 1.0, 1.9), (0.1, 1.0, 1.4896)]
# the points at which the reference's sample_visible = true density is biased beyond 6 standard errors (measured: 540, 96 and 395 standard
# errors, -28 %, -4 % and -25 % of the albedo; at (0.9, 0.05, 1.5) G1(wi) is 1 to 1e-3 and the two densities nearly agree: 0.7 standard errors)
BIASED = [(0.1, 0.3, 1.5), (0.5, 1.0, 1.9), (0.1, 1.0, 1.4896)]
RHO, S = 0.5, 1.0
SSW = S / (S + RHO)


@functools.lru_cache(maxsize=None)
def contract_point(cos_i, alpha, eta):
    lo, hi = (RP.albedo64(cos_i, RHO, S, eta, alpha, False, order) for order in (12, 20))
    assert abs(lo - hi) <= 1e-6 * hi, (cos_i, alpha, eta, lo, hi)       # the quadrature has converged: two orders agree
    return hi


@pytest.mark.parametrize("cos_i,alpha,eta", POINTS)
def test_the_contract_is_unbiased_in_float64(cos_i, alpha, eta):
    """the mean of sample()'s weights over 2^20 stratified (sample1, u) within 6 of its own standard errors of the Gauss-Legendre
    integral of eval over the hemisphere; the integral of pdf is 1 minus the mass the coat's sampling sends below the horizon"""
    want = contract_point(cos_i, alpha, eta)
    w = RP.sample_weights64(cos_i, RHO, S, eta, alpha, SSW, False)
    # the standard error of independent samples, from the plain sample variance: the samples are stratified, so the true error is
    # smaller and the bound looser than it reads (measured deviations: 0.03 to 0.25 of this figure).  The bias test below uses the
    # same figure and still separates by 96 to 543 of it.
    mean, se = w.mean(), w.std(ddof=1) / np.sqrt(len(w))
    print("ROUGHPLASTIC contract cos_i %g alpha %g eta %g: albedo %.9g mean %.9g se %.3g (%.2f se)" % (cos_i, alpha, eta, want, mean, se, (mean - want) / se))
    assert len(w) == 1 << 20 and abs(mean - want) <= 6 * se and se < 1e-3 * want
    m12, m20 = (RP.pdf_mass64(cos_i, eta, alpha, SSW, order) for order in (12, 20))
    ps = RP.lobes64(cos_i, eta, SSW)[1]
    below = RP.coat_mass_below64(cos_i, alpha)
    print("ROUGHPLASTIC pdf mass %.12g, 1 - ps * below %.12g (ps %.6g below %.6g)" % (m20, 1.0 - ps * below, ps, below))
    assert abs(m12 - m20) <= 1e-6 * m20 and m20 <= 1.0 + 1e-12
    assert abs(m20 - (1.0 - ps * below)) <= 1e-6
    assert abs(below - RP.coat_mass_below64(cos_i, alpha, panels=32768)) <= 1e-7          # (the rule over the normal has converged too)


def test_the_visible_normal_density_of_the_reference_is_biased():
    """the same estimator with roughplastic.cpp:144-146's density under sample_visible = true, the normal still drawn from
    D(m) cos(theta_m) (microfacet.h:131-143): beyond 6 standard errors at BIASED — why the flag is refused (msk_gpu.h, the departure)"""
    far = []
    for cos_i, alpha, eta in POINTS:
        want = contract_point(cos_i, alpha, eta)
        w = RP.sample_weights64(cos_i, RHO, S, eta, alpha, SSW, False, visible=True)
        mean, se = w.mean(), w.std(ddof=1) / np.sqrt(len(w))
        print("ROUGHPLASTIC sample_visible cos_i %g alpha %g eta %g: albedo %.9g mean %.9g (%.1f se, %.2f %%)" % (cos_i, alpha, eta, want, mean, (mean - want) / se, 100 * (mean / want - 1)))
        if abs(mean - want) > 6 * se:
            far.append((cos_i, alpha, eta))
    assert far == BIASED


# ===================================================================================================== CPU 3: native, layout, plan
@pytest.fixture(scope="module")
def native_exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("roughplastic_tables")
    src = os.path.join(ROOT, "tests", "native", "roughplastic_tables_check.cpp")
    plain, san = str(d / "roughplastic_tables_check"), str(d / "roughplastic_tables_check_san")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", plain, src])
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", san, src])
    return plain, san


def test_native_packer_check(native_exe):
    """every refusal text, type 5's words, alpha_u != alpha_v, the record of a type 7, type 6's record and a scene without a plastic to
    their recorded digests, the constants against float64: plain and sanitized"""
    for exe in native_exe:
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stdout.split()[0] == "ok", r.stdout[-2000:] + r.stderr[-2000:]


@pytest.mark.parametrize("knobs", LP.KNOB_SETS, ids=lambda k: ",".join(f"{a}={b}" for a, b in k.items()) or "defaults")
def test_plan_with_a_roughplastic(native_exe, knobs):
    """a packed type-7 scene plans SHADE_MASK (the _m kernels), or SHADE_LENS (_l) with a lens, with and without a mask of its own"""
    env = {k: v for k, v in os.environ.items() if not k.startswith("MSK_")}
    env.update(knobs)
    r = subprocess.run([native_exe[0], "plan"], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    assert r.stdout.split() == ["cases", str(2 * 2 * 7 * 64)]


def test_exports_and_struct_layouts(abi, tmp_path):
    src = tmp_path / "off.c"
    names = ("type", "back_bsdf", "reflectance", "alpha_u", "alpha_v", "sample_visible", "eta", "k", "specular_reflectance", "specular_transmittance", "ior_eta",
             "ior_inv_eta", "reflectance_texture", "reflectance_scale", "reflectance_regular")
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "msk_gpu.h"\nint main(){printf("%zu ' + "%zu " * len(names) + '%d %d %d\\n",sizeof(msk_bsdf_desc),'
                   + ",".join("offsetof(msk_bsdf_desc,%s)" % n for n in names) + ',MSK_BSDF_PLASTIC,MSK_BSDF_ROUGHPLASTIC,MSK_ABI_VERSION);return 0;}\n')
    exe = tmp_path / "off"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    b = abi.BsdfDesc
    assert got == [C.sizeof(b)] + [getattr(b, n).offset for n in names] + [abi.MSK_BSDF_PLASTIC, abi.MSK_BSDF_ROUGHPLASTIC, abi.MSK_ABI_VERSION]
    assert got[0] == 132 and got[-3:] == [6, 7, 8]                       # the descriptor keeps its size; type 5 stays unassigned; ABI v8
    import __graft_entry__ as ge
    ge.build_gpu_library()
    lib = C.CDLL(abi.LIB_PATH)
    for name in ("msk_gpu_roughplastic_sample", "msk_gpu_roughplastic_eval", "msk_gpu_plastic_constants"):
        assert name in abi.EXPORTS and getattr(lib, name) is not None


# ===================================================================================================== CPU 4: the two flatteners
def flattener_meshes(hm):
    return [quad(hm, "defaults", {"type": "roughplastic"}, 0.0),
            quad(hm, "twosided", roughplastic((0.2, 0.5, 0.7), (0.9, 0.8, 0.6), 1.9, True, 0.05, twosided=True), 0.1),
            quad(hm, "masked", {"type": "mask", "opacity": 0.375, "bsdf": roughplastic(0.25, 0.5, 1.2, alpha=1.0, twosided=True)}, 0.2),
            quad(hm, "bitmap", roughplastic(dict(TP.BITMAP), 0.7, nonlinear=True, alpha=(0.25, 0.25), distribution="ggx", sample_visible=False), 0.3, uv=True),
            quad(hm, "checker", roughplastic(dict(TP.CHECKER), (0.5, 0.5, 0.5), alpha=1e-5), 0.4, uv=True),
            quad(hm, "iors", {"type": "roughplastic", "int_ior": 1.33, "ext_ior": 1.1, "specular_reflectance": 2.0}, 0.5)]


def test_the_two_flatteners_agree(hostmirror, abi, tmp_path):
    """XML through the C++ host against the dict through the Python mirror: the same descriptors byte for byte (defaults, `twosided`,
    `mask` over it, a bitmap and a checkerboard base, equal alpha_u / alpha_v); `beckmann`, `sample_visible`, unequal alphas and a
    textured specular_reflectance refused in the same words"""
    hostlib = EV.host_library()
    xml = hostmirror.write_scene_xml(flattener_meshes(hostmirror), str(tmp_path / "s"), 16, 16, 1, camera=CAM)
    text = open(xml).read()
    assert text.count('<bsdf type="roughplastic">') == 6 and text.count('<bsdf type="twosided">') == 2 and text.count('<bsdf type="mask">') == 1
    assert text.count('name="alpha_u"') == 1 and text.count('name="sample_visible"') == 1 and text.count('name="distribution"') == 1
    h = hostlib.HostScene(xml).flatten()
    m = hostmirror.flatten(flattener_meshes(hostmirror), 16, 16, camera=CAM, coeff_lookup=hostlib.srgb_model_fetch)
    assert h.desc.n_bsdfs == m.desc.n_bsdfs == 6 and h.desc.n_textures == m.desc.n_textures == 2
    for i in range(6):
        assert bytes(h.desc.bsdfs[i]) == bytes(m.desc.bsdfs[i]), i
        assert m.desc.bsdfs[i].type == abi.MSK_BSDF_ROUGHPLASTIC
    for i in range(2):
        assert bytes(h.desc.textures[i]) == bytes(m.desc.textures[i]), i
    assert len(h.masks) == len(m.masks) == 1 and h.masks[0].bsdf == m.masks[0].bsdf == 2 and h.masks[0].opacity == m.masks[0].opacity == 0.375
    d = m.desc.bsdfs
    assert (d[0].reflectance_scale, d[0].specular_reflectance.scale, d[0].sample_visible, d[0].back_bsdf) == (0.5, 1.0, 0, -1)
    assert d[0].alpha_u == d[0].alpha_v == F(0.1) and d[0].ior_eta == F(1.49) / F(1.00028) and d[0].ior_inv_eta == F(1.00028) / F(1.49)
    assert (d[1].back_bsdf, d[1].sample_visible, d[2].back_bsdf) == (1, 1, 2) and d[1].alpha_u == d[1].alpha_v == F(0.05) and d[2].alpha_u == 1.0
    assert (d[3].reflectance_texture, d[4].reflectance_texture, d[3].sample_visible) == (1, 2, 1) and d[3].alpha_u == d[3].alpha_v == 0.25
    assert d[4].alpha_u == F(1e-5) and d[5].ior_eta == F(1.33) / F(1.1) and d[5].specular_reflectance.scale == 2.0
    # the refusals, worded alike
    plain = hostmirror.write_scene_xml([quad(hostmirror, "q", None)], str(tmp_path / "r"), 16, 16, 1, camera=CAM)
    text = open(plain).read()
    start, end = text.index("<bsdf"), text.index("</bsdf>") + len("</bsdf>")
    tex = '<texture name="specular_reflectance" type="checkerboard"><rgb name="color0" value="0.1"/><rgb name="color1" value="0.2"/></texture>'
    cases = [(tex, roughplastic(0.5, dict(TP.CHECKER)), hostmirror.ROUGHPLASTIC_SPECULAR),
             ('<string name="distribution" value="beckmann"/>', roughplastic(distribution="beckmann"), hostmirror.ROUGHPLASTIC_BECKMANN),
             ('<string name="distribution" value="phong"/>', roughplastic(distribution="phong"), hostmirror.ROUGHPLASTIC_DISTRIBUTION % "phong"),
             ('<boolean name="sample_visible" value="true"/>', roughplastic(sample_visible=True), hostmirror.ROUGHPLASTIC_VISIBLE),
             ('<float name="alpha_u" value="0.1"/><float name="alpha_v" value="0.2"/>', roughplastic(alpha=(0.1, 0.2)), hostmirror.ROUGHPLASTIC_ANISOTROPIC)]
    for k, (body, spec, words) in enumerate(cases):
        path = tmp_path / "r" / ("bad%d.xml" % k)
        path.write_text(text[:start] + '<bsdf type="roughplastic">' + body + '</bsdf>' + text[end:])
        with pytest.raises(hostlib.HostError) as e:
            hostlib.HostScene(str(path)).flatten()
        assert words in str(e.value), (k, str(e.value))
        with pytest.raises(ValueError) as e:
            hostmirror.flatten([quad(hostmirror, "q", spec)], 16, 16, camera=CAM)
        assert words in str(e.value), (k, str(e.value))
        xml_k = open(hostmirror.write_scene_xml([quad(hostmirror, "q", spec)], str(tmp_path / ("w%d" % k)), 16, 16, 1, camera=CAM)).read()
        with pytest.raises(hostlib.HostError) as e:                      # ... and through the mirror's own XML
            hostlib.HostScene(os.path.join(str(tmp_path / ("w%d" % k)), os.path.basename(plain))).flatten()
        assert words in str(e.value) and '<bsdf type="roughplastic">' in xml_k, (k, str(e.value))
    assert hostmirror.ROUGHPLASTIC_SPECULAR.startswith('roughplastic: "specular_reflectance"') and "anisotropic" in hostmirror.ROUGHPLASTIC_ANISOTROPIC
    assert "biases sample = eval / pdf" in hostmirror.ROUGHPLASTIC_VISIBLE


# ===================================================================================================== float64 expectations
def local(v):
    """world -> the plane's shading frame (normal +y); the BSDF is isotropic, so any tangent pair serves"""
    v = np.asarray(v, np.float64)
    return np.stack([v[..., 0], v[..., 2], v[..., 1]], -1)


@functools.lru_cache(maxsize=None)
def coat_albedo(cos_i, eta, alpha, order=12, panels=32):
    """the integral of the coat's lobe with s = 1 (the base is black)"""
    return RP.albedo64(float(cos_i), 0.0, 1.0, eta, alpha, False, order, panels)


def base_spectrum(desc, nonlinear, b=0):
    bd = desc.bsdfs[b]
    fdr = P.fdr_int64(float(bd.ior_eta))
    rho = D.sigmoid_spectrum(bd.reflectance[:], bd.reflectance_scale)
    return rho.map((lambda r: r / (1.0 - fdr * r)) if nonlinear else (lambda r: r / (1.0 - fdr))) * (1.0 - fdr)


def sky_value(flat, m, s, nonlinear, alpha, order=12, panels=32):
    """L albedo(wi) over the crop: the coat's integral by quadrature, the base's (1 - F_i) D (1 - fdr_int) as for the plastic"""
    desc = flat.desc
    eta = float(desc.bsdfs[0].ior_eta)
    c, w = TP.crop_cosines(desc, m)[:2]
    coat = sum(wk * coat_albedo(ck, eta, alpha, order, panels) for ck, wk in zip(c.ravel(), w.ravel())) * s
    base = float((w * (1.0 - P.fresnel64(c, eta))).sum())
    sky = D.emitter_spectrum(desc, 0)
    cie = DM.cie_of(desc)
    return R.expected_xyz(sky, cie) * coat + R.expected_xyz(sky * base_spectrum(desc, nonlinear), cie) * base


def sun_value(flat, d, rho, s, nonlinear, alpha):
    """E eval(wi, wo_sun) pointwise, per unit of the sun's irradiance spectrum, for view directions d [..., 3]"""
    eta = float(flat.desc.bsdfs[0].ior_eta)
    wo = local(-SD.light_of(flat, 0)[1])
    assert wo[2] > 0
    return RP.eval64(local(-d), wo, rho, s, eta, alpha, nonlinear)


COLOUR = (0.7, 0.4, 0.2)


def closed_form_case(hm, name, fine=False):
    """-> (flat, expectation, render parameters); fine: more crop nodes and a finer rule over the hemisphere"""
    kind = name.split("_")[0]
    m, order, panels = (8, 16, 48) if fine else (4, 12, 32)
    if kind == "a":
        cam = STEEP if "steep" in name else GRAZING
        nonlinear, alpha = "nonlinear" in name, 0.1 if "steep" in name else 0.3
        flat = hm.flatten([DM.plane(hm, roughplastic(COLOUR, 0.7, 1.4896, nonlinear, alpha))], W48, W48, camera=cam, env=SKY, coeff_lookup=EV.host_library().srgb_model_fetch)
        c = TP.crop_cosines(flat.desc, 4)[0]
        assert (c.min() > 0.9) if cam is STEEP else (c.max() < 0.2)
        return flat, sky_value(flat, m, 0.7, nonlinear, alpha, order, panels), dict(max_depth=2)
    if kind == "b":
        flat = hm.flatten([DM.plane(hm, roughplastic(0.5, 0.7, 1.4896, True, 0.3))], W48, W48, camera=CAM, lights=[SD.sun_spec()])
        o, d, w = DM.crop_rays(flat.desc, m)
        return flat, TP.sky_xyz(flat.desc) * float((w * sun_value(flat, d, 0.5, 0.7, True, 0.3)).sum()), dict(max_depth=2)
    if kind == "c":
        flat = hm.flatten([DM.plane(hm, roughplastic(0.0, 1.0, 1.4896, False, 0.3))], W48, W48, camera=STEEP, env=SKY)
        return flat, sky_value(flat, m, 1.0, False, 0.3, order, panels), dict(max_depth=2)
    if kind == "d":                                                     # the rough coat tends to the smooth one: the plastic's closed form
        flat = hm.flatten([DM.plane(hm, roughplastic(0.5, 0.7, 1.4896, True, 1e-4))], W48, W48, camera=CAM, env=SKY)
        return flat, TP.sky_xyz(flat.desc) * TP.grey_value(flat.desc, m, 0.5, 0.7, True), dict(max_depth=2)
    raise KeyError(name)


CASES = ["a_steep_linear", "a_steep_nonlinear", "a_grazing_linear", "a_grazing_nonlinear", "b_sun", "c_coat_alone", "d_alpha_1e-4_is_the_plastic"]


@pytest.mark.parametrize("name", CASES)
def test_expectations_have_converged(hostmirror, name):
    """4 x 4 crop nodes and the 32-panel order-12 rule over the hemisphere against 8 x 8 nodes and 48 panels of order 16"""
    _, e, _ = closed_form_case(hostmirror, name)
    _, fine, _ = closed_form_case(hostmirror, name, fine=True)
    print("ROUGHPLASTIC %s: expectation %s (fine: %s)" % (name, e, fine))
    assert np.all(e > 0) and np.all(np.abs(e - fine) <= 1e-5 * fine)


def film_case(hm, name, m=10):
    """(a), (b) on DM.film_case's 32 x 32 film: (flat, expectation of sum XYZ / sum W, effective samples / samples)"""
    if name == "a":
        flat = hm.flatten([DM.plane(hm, roughplastic(0.5, 0.7, 1.4896, True, 0.3))], 32, 32, camera=CAM, env=SKY)
        eta = float(flat.desc.bsdfs[0].ior_eta)
        base = P.base64(0.5, eta, True) * (1.0 - P.fdr_int64(eta))

        def value(o, d):
            c = -d[..., 1]
            return 0.7 * np.vectorize(lambda ck: coat_albedo(ck, eta, 0.3, 12, 16))(c) + (1.0 - P.fresnel64(c, eta)) * base
    else:
        flat = hm.flatten([DM.plane(hm, roughplastic(0.5, 0.7, 1.4896, True, 0.3))], 32, 32, camera=CAM, lights=[SD.sun_spec()])
        value = lambda o, d: sun_value(flat, d, 0.5, 0.7, True, 0.3)
    t, a, n_eff = DM.film_weights(flat.desc, 32, m)
    yy, xx = np.meshgrid(t, t, indexing="ij")
    o, d = R.camera_ray(flat.desc, xx, yy)
    return flat, TP.sky_xyz(flat.desc) * float(np.einsum("j,k,jk->", a, a, value(o, d))), n_eff


@pytest.mark.parametrize("name", ["a", "b"])
def test_film_expectations_have_converged(hostmirror, name):
    _, fine, n_eff = film_case(hostmirror, name, 14)
    _, coarse, _ = film_case(hostmirror, name, 10)
    print("ROUGHPLASTIC film %s: fine %s coarse %s effective samples / samples %.4f" % (name, fine, coarse, n_eff))
    assert np.all(np.abs(coarse - fine) <= 1e-5 * fine) and 0.8 < n_eff < 1.0
    if name == "a":                                                      # (the 16-panel rule the film's nodes use against the crop's 32)
        assert abs(coat_albedo(0.35, 1.4896, 0.3, 12, 16) - coat_albedo(0.35, 1.4896, 0.3, 12, 32)) <= 1e-7


# ===================================================================================================== GPU 1: the probes
def probe_entries():
    """(name, spec): alpha 1e-5 (clamped), 0.05, 0.3 and 1; both `nonlinear`; a bitmap and a checkerboard base; s = 0 (ps = 0: never the
    coat) and rho = 0 (pd = 0: always the coat); one-sided and twosided"""
    return [("clamped", roughplastic((0.6, 0.5, 0.4), (0.9, 0.8, 0.7), 1.4896, False, 1e-5)),
            ("a005_nonlinear", roughplastic((0.9, 0.95, 0.99), 0.7, 1.4896, True, 0.05, twosided=True)),
            ("a03", roughplastic((0.6, 0.5, 0.4), (0.9, 0.8, 0.7), 1.9, False, 0.3)),
            ("a1_nonlinear", roughplastic((0.3, 0.6, 0.2), 0.7, 1.9, True, 1.0, twosided=True)),
            ("bitmap", roughplastic(dict(TP.BITMAP), 0.7, 1.4896, True, 0.3)),
            ("checker", roughplastic(dict(TP.CHECKER), (0.5, 0.6, 0.7), 1.2, False, 0.05, twosided=True)),
            ("no_coat", roughplastic(0.5, 0.0, 1.9, True, 0.3)),
            ("black_base", roughplastic(0.0, 0.7, 1.4896, True, 0.05))]


N_PROBE = 125                                                            # per entry: 8 x 125 = 1000 inputs, neither a multiple of 64


def probe_inputs(rng, n, ps_of):
    uv = rng.uniform(-1.5, 1.5, (n, 2)).astype(F)
    wi = rng.normal(size=(n, 3))
    wi = (wi / np.linalg.norm(wi, axis=1, keepdims=True)).astype(F)
    wi[0::16] = [0, 0, 1]
    wi[1::16] = [1, 0, 0]                                                # cos_i = 0
    wi[2::16, 2] = -np.abs(wi[2::16, 2])                                 # a negative cos_i
    z = F(1e-3)
    wi[3::16] = [np.sqrt(F(1) - z * z), 0, z]                            # cos_i = 1e-3
    wo = rng.normal(size=(n, 3))
    wo = (wo / np.linalg.norm(wo, axis=1, keepdims=True)).astype(F)
    wo[4::16] = [0, 1, 0]
    wo[5::16] = wi[5::16] * np.array([-1, -1, 1], F)                     # the mirror direction: H = n
    su = rng.uniform(0, 1, (n, 3)).astype(F)
    su[8::16, 1], su[9::16, 1] = 0, ONE_BELOW                            # u.x at both ends
    su[10::16, 2], su[11::16, 2] = 0, ONE_BELOW
    ps = ps_of(wi)                                                       # sample1 on both sides of ps and equal to it
    su[5::8, 0], su[6::8, 0], su[7::8, 0] = ps[5::8], np.nextafter(ps[6::8], F(-1)), np.nextafter(ps[7::8], F(2))
    su[12::16, 0] = 0                                                    # the coat wherever ps > 0
    su[:, 0] = np.clip(np.nan_to_num(su[:, 0], nan=0.5), 0, ONE_BELOW)
    wl = rng.uniform(360, 830, (n, 4)).astype(F)
    return uv, wi, wo, su, wl


@pytest.mark.gpu
def test_probes_equal_the_restatement_bit_for_bit(gpu_ctx, oracle, hostmirror, abi):
    """(1) msk_gpu_roughplastic_sample / msk_gpu_roughplastic_eval against roughplastic_ref, given the constants
    msk_gpu_plastic_constants returns (held to float64 here with the plastic's bounds).  8 entries x 125 inputs"""
    entries = probe_entries()
    meshes = [quad(hostmirror, name, spec, 0.1 * i, uv=True) for i, (name, spec) in enumerate(entries)]
    meshes.append(hostmirror.MeshSpec("lamp", [tuple(DM.LAMP)], hostmirror.LUMINAIRE, radiance=(40, 30, 20)))
    meshes.append(quad(hostmirror, "smooth", TP.plastic(), 0.1 * len(entries)))
    flat = hostmirror.flatten(meshes, 16, 16, camera=CAM, coeff_lookup=None)
    g = abi.Scene(gpu_ctx, flat)
    rng = np.random.RandomState(13)
    seen = dict(coat=0, base=0, dead=0, failed=0)
    try:
        for b, (name, spec) in enumerate(entries):
            bd = flat.desc.bsdfs[b]
            assert bd.type == abi.MSK_BSDF_ROUGHPLASTIC
            fdr, ssw = g.plastic_constants(b)
            eta, inv_eta, nonlinear, alpha = F(bd.ior_eta), F(bd.ior_inv_eta), bool(bd.sample_visible), F(bd.alpha_u)
            want_fdr, want_ssw = P.fdr_int64(float(eta)), P.desc_ssw64(flat.desc, b, flat.texels)
            assert abs(float(fdr) - want_fdr) <= 2e-7 * want_fdr and abs(float(ssw) - want_ssw) <= 1e-6, (name, fdr, want_fdr, ssw, want_ssw)
            assert (ssw == 1.0) if name == "black_base" else (ssw == 0.0) if name == "no_coat" else 0 < ssw < 1
            twosided = bd.back_bsdf >= 0

            def front(w):
                return np.where((w[:, 2:3] < 0) & twosided, w * np.array([1, 1, -1], F), w).astype(F), (w[:, 2] < 0) & twosided

            uv, wi, wo_in, su, wl = probe_inputs(rng, N_PROBE, lambda w: P.lobes32(front(w)[0][:, 2], eta, ssw)[2])
            wif, flipped = front(wi)
            rho = TP.rho32(oracle, flat, b, uv, wl)
            s = D.spectrum32(oracle if not np.isinf(bd.specular_reflectance.coeff[2]) else None, bd.specular_reflectance, wl)
            hemi = np.array([oracle.warps(u)[2] for u in su[:, 1:]], F)
            want = RP.sample32(oracle, wif, su[:, 0], su[:, 1:], hemi, rho, s, eta, inv_eta, fdr, ssw, nonlinear, alpha)
            want["wo"][flipped, 2] = -want["wo"][flipped, 2]
            wo_pdf, value, flags = g.roughplastic_sample(b, uv, wi, su, wl)
            assert np.array_equal(flags[:, 3] != 0, want["ok"]), name
            assert not flags[:, 1].any() and not flags[:, 2].any() and np.all(flags[:, 0] == 1)      # never delta, no null lobe, eta = 1
            for what, got, ref in (("wo", wo_pdf[:, :3], want["wo"]), ("pdf", wo_pdf[:, 3], want["pdf"]), ("value", value, want["value"])):
                bad = (bits(got) != bits(ref)).reshape(len(wi), -1).any(-1) & ~((got == 0) & (ref == 0)).reshape(len(wi), -1).all(-1)
                assert not bad.any(), (name, what, int(bad.sum()), got[bad][:3], ref[bad][:3], wi[bad][:3], su[bad][:3])
            live = want["pdf"] > 0
            seen["coat"] += int((want["coat"] & live).sum()); seen["base"] += int((~want["coat"] & live).sum())
            seen["dead"] += int((want["coat"] & ~live).sum()); seen["failed"] += int((~want["ok"]).sum())
            if name == "no_coat":
                assert not want["coat"].any()
            if name == "black_base":
                assert want["coat"][want["ok"]].all()
            a_pdf, ev = g.roughplastic_eval(b, uv, wi, wo_in, wl)
            wof = np.where(flipped[:, None], wo_in * np.array([1, 1, -1], F), wo_in).astype(F)
            rv, rp = RP.eval32(wif, wof, rho, s, eta, inv_eta, fdr, ssw, nonlinear, alpha)
            assert np.all(a_pdf[:, 0] == 1)
            for what, got, ref in (("eval", ev, rv), ("eval pdf", a_pdf[:, 1], rp)):
                bad = (bits(got) != bits(ref)).reshape(len(wi), -1).any(-1)
                assert not bad.any(), (name, what, int(bad.sum()), got[bad][:3], ref[bad][:3], wi[bad][:3], wo_in[bad][:3])
            assert rp.max() > 0
        print("ROUGHPLASTIC probes: %s" % seen)
        assert min(seen.values()) > 0
        lamp, smooth = len(entries), len(entries) + 1
        for call in (lambda: g.roughplastic_sample(lamp, uv[:1], wi[:1], su[:1], wl[:1]), lambda: g.roughplastic_eval(smooth, uv[:1], wi[:1], wo_in[:1], wl[:1]),
                     lambda: g.roughplastic_sample(smooth + 1, uv[:1], wi[:1], su[:1], wl[:1])):
            with pytest.raises(abi.MskError) as err:
                call()
            assert err.value.code == abi.MSK_ERR_INVALID_ARG and ("not a roughplastic of this scene" in str(err.value) or "out of range" in str(err.value))
        with pytest.raises(abi.MskError) as err:                         # ... and the plastic's probes refuse a roughplastic
            g.plastic_sample(0, uv[:1], wi[:1], su[:1], wl[:1])
        assert "not a plastic of this scene" in str(err.value)
        with pytest.raises(abi.MskError) as err:
            g.plastic_constants(lamp)
        assert "not a plastic of this scene" in str(err.value)
        assert g.plastic_constants(smooth)[0] == g.plastic_constants(0)[0]      # the same eta, the same fdr_int, each from its own words
    finally:
        g.close()


# ===================================================================================================== GPU 2: float64 expectations
@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_rendered_radiance_meets_the_expectation(gpu_ctx, hostmirror, abi, name):
    """(a) a coloured plane under the sky = L albedo(wi), steep and grazing, linear and nonlinear; (b) a sun: E eval(wi, wo_sun), the
    next-event path alone; (c) the coat alone; (d) alpha 1e-4 against the plastic's closed form: |mean - E| <= 6 standard errors +
    1e-3 E per channel"""
    flat, expected, params = closed_form_case(hostmirror, name)
    g = abi.Scene(gpu_ctx, flat)
    try:
        mean, se = TP.sampled_mean(g, abi, name, expected, **params)
    finally:
        g.close()
    assert np.all(np.abs(mean - expected) <= 6 * se + 1e-3 * expected), ((mean - expected) / expected, se / expected)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["a", "b"])
def test_film_in_pcg_block_mode_meets_the_expectation(gpu_ctx, hostmirror, abi, name):
    """(a), (b) under MSK_RNG_PCG_BLOCK (k_path_serial_m) through a 32 x 32 film, by test_plastic_bsdf's procedure"""
    flat, expected, n_eff = film_case(hostmirror, name)
    g = abi.Scene(gpu_ctx, flat)
    px = np.array([(x, y) for y in range(32) for x in range(32)], np.int32)
    xyz, _ = g.sample_pixels(abi.render_params(spp=64, seed=9, max_depth=2), px)
    sigma = np.sqrt(xyz.astype(np.float64).var(1, ddof=1).mean(0))
    spp = 256
    film, st = g.render(EV.pcg(abi, spp=spp, seed=7, max_depth=2))
    g.close()
    assert st.samples == 32 * 32 * spp
    f = film.astype(np.float64)
    mean = f[..., :3].sum((0, 1)) / f[..., 4].sum()
    se = sigma / np.sqrt(n_eff * st.samples)
    print("ROUGHPLASTIC film %s: expected %s mean %s se/|E| %s dev/|E| %s" % (name, expected, mean, se / expected, (mean - expected) / expected))
    assert np.all(se <= 5e-3 * expected)
    assert np.all(np.abs(mean - expected) <= 6 * se + 1e-3 * expected)


# ===================================================================================================== GPU 3: identities
def variant_meshes(hm, pads=(), masked=False):
    """test_plastic_bsdf's box with the two plastics made rough: alpha 0.05 over the bitmap base, the default 0.1 on the short box"""
    meshes = TP.variant_meshes(hm, pads, masked)
    for m in meshes:
        spec = m.bsdf["bsdf"] if isinstance(m.bsdf, dict) and m.bsdf.get("type") == "mask" else m.bsdf
        if isinstance(spec, dict) and spec.get("type") == "plastic":
            spec["type"] = "roughplastic"
            if m.name == "cbox_largebox":
                spec["alpha"] = 0.05
    return meshes


def variant_flat(hm, which, crop=None, masked=False, lens=False):
    kw = dict(env=SKY, points=[DM.BOX_POINT], crop=crop)
    if lens:
        kw["camera"] = dict(hm.CBOX_CAMERA, aperture_radius=0.0, focus_distance=500.0)
    if which == "lds":
        return hm.flatten(variant_meshes(hm, masked=masked), 48, 48, **kw)
    filler = hm.blob_mesh("filler", (150, 420, 400), 60, 16, 16, hm.WHITE, seed=9)
    base = hm.flatten(variant_meshes(hm, [filler], masked=masked), 48, 48, **kw)
    pads = T.faceless_pads(hm, T.SMALL_TABLES_F4 + 1 - T.table_plan(base)["small_f4"])
    return hm.flatten(variant_meshes(hm, [filler] + pads, masked=masked), 48, 48, **kw)


def render_three(g, abi):
    xyz, pos = g.sample_pixels(abi.render_params(spp=16, seed=5), EV.crop_pixels())
    film, st = g.render(abi.render_params(spp=8, seed=5))
    serial, _ = g.render(EV.pcg(abi, spp=2, seed=5))
    return xyz, pos, film, serial, st


@pytest.fixture(scope="module")
def variant_reference(gpu_ctx, hostmirror, abi):
    """the default variant's samples and films of the two scenes (no knob set): computed once, never changed"""
    saved = {k: os.environ.pop(k) for k in DM.KNOBS if k in os.environ}
    out = {}
    try:
        for which in ("lds", "hbm"):
            flat = variant_flat(hostmirror, which)
            assert sum(flat.desc.bsdfs[i].type == abi.MSK_BSDF_ROUGHPLASTIC for i in range(flat.desc.n_bsdfs)) == 2
            g = abi.Scene(gpu_ctx, flat)
            xyz, pos, film, serial, st = render_three(g, abi)
            g.close()
            for a in (xyz, pos, film, serial):
                a.setflags(write=False)
            assert np.isfinite(film).all() and film[..., :3].max() > 0
            out[which] = dict(flat=flat, xyz=xyz, pos=pos, film=film, serial=serial, samples=st.samples)
    finally:
        os.environ.update(saved)
    return out


# mskplan::TraceMode (csrc/msk_plan.h): the tree a scene's traversal kernels walk
BIN_LDS, BIN_HBM, WIDE4, WIDE4_LDS, WIDE8, WIDE4_BYTE, WIDE4_HALF = range(7)
# (scene, knobs, the tree form the knobs must give).  MSK_WIDE_BVH and MSK_QUANT_BVH are read only for a tree in HBM (place_tree), so each
# stands beside MSK_LDS_SCENE_KB=0.  Every form the library walks by default or by a documented knob is here; TRACE_WIDE4_LDS, the
# MSK_WIDE_LDS experiment that is off by default, is not.
VARIANTS = [("lds", {"MSK_STREAMS": "1"}, BIN_LDS), ("lds", {"MSK_FUSED": "1"}, BIN_LDS), ("lds", {"MSK_SORT": "0"}, BIN_LDS), ("lds", {"MSK_BVH_BUILD": "gpu"}, BIN_LDS),
            ("lds", {"MSK_LDS_SCENE_KB": "0"}, WIDE4_HALF), ("lds", {"MSK_LDS_SCENE_KB": "0", "MSK_WIDE_BVH": "8"}, WIDE8),
            ("lds", {"MSK_LDS_SCENE_KB": "0", "MSK_WIDE_BVH": "0"}, BIN_HBM), ("lds", {"MSK_LDS_SCENE_KB": "0", "MSK_QUANT_BVH": "0"}, WIDE4),
            ("lds", {"MSK_LDS_SCENE_KB": "0", "MSK_QUANT_BVH": "1"}, WIDE4_BYTE),
            ("hbm", {"MSK_LDS_SCENE_KB": "0"}, WIDE4_HALF), ("hbm", {"MSK_LDS_SCENE_KB": "0", "MSK_FUSED": "1"}, WIDE4_HALF),
            ("hbm", {"MSK_LDS_SCENE_KB": "0", "MSK_SORT": "0", "MSK_STREAMS": "1"}, WIDE4_HALF),
            ("hbm", {"MSK_LDS_SCENE_KB": "0", "MSK_QUANT_BVH": "1", "MSK_BVH_BUILD": "gpu"}, WIDE4_BYTE),
            ("hbm", {"MSK_LDS_SCENE_KB": "0", "MSK_WIDE_BVH": "8", "MSK_BVH_BUILD": "gpu"}, WIDE8), ("hbm", {"MSK_LDS_SCENE_KB": "0", "MSK_WIDE_BVH": "0"}, BIN_HBM),
            ("hbm", {"MSK_LDS_SCENE_KB": "0", "MSK_QUANT_BVH": "0"}, WIDE4)]      # (the fused HBM kernel walks the half-float form only: no MSK_FUSED here)
variant_ids = lambda v: EV.variant_id(v) if isinstance(v, dict) else str(v)


@pytest.fixture(scope="module")
def tree_form(tmp_path_factory, abi):
    """tests/native/direct_plan_probe.cpp (test_direct_oracle_parity's probe: pack, build, place_tree as msk_gpu_scene_create runs them, the
    knobs read from the environment) -> the TraceMode of a flattened scene under the knobs now set.  MSK_BVH_BUILD=gpu builds the tree on
    the device; the host builder's tree stands in for its size here, which the form of these scenes does not hang on (both scenes are far
    from the MSK_LDS_SCENE_KB limit on either side of it)."""
    so = str(tmp_path_factory.mktemp("tree_form") / "direct_plan_probe.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", os.path.join(ROOT, "include"), "-o", so,
                           os.path.join(ROOT, "tests", "native", "direct_plan_probe.cpp")])
    lib = C.CDLL(so)

    def probe(flat):
        pts = flat.points
        pts = (abi.PointDesc * len(pts))(*pts) if isinstance(pts, (list, tuple)) else pts
        em = abi.SceneMasks(abi.SceneExt(None, len(pts) if pts is not None else 0, pts), 0, None)
        out, msg = (C.c_int64 * 10)(), C.create_string_buffer(512)
        rc = lib.direct_plan_probe(C.byref(flat.desc), C.byref(em), 1, 1, C.c_uint64(4096), out, msg, 512)
        assert rc == 0, msg.value
        return int(out[2])
    return probe


def set_knobs(monkeypatch, env):
    for k in DM.KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def test_the_variants_walk_every_tree_form(hostmirror, tree_form, monkeypatch):
    """the plan of every entry of VARIANTS, by the library's own placement code on the scenes themselves: each knob set gives the tree
    form the list names, the defaults stage the `lds` scene's tree in LDS, and the list covers all six forms"""
    flats = {which: variant_flat(hostmirror, which) for which in ("lds", "hbm")}
    set_knobs(monkeypatch, {})
    assert tree_form(flats["lds"]) == BIN_LDS
    for which, env, form in VARIANTS:
        set_knobs(monkeypatch, env)
        assert tree_form(flats[which]) == form, (which, env, tree_form(flats[which]))
    set_knobs(monkeypatch, {"MSK_WIDE_BVH": "8", "MSK_QUANT_BVH": "1"})       # (alone the two knobs do nothing to a tree in LDS: why they are paired)
    assert tree_form(flats["lds"]) == BIN_LDS
    assert {form for _, _, form in VARIANTS} == {BIN_LDS, BIN_HBM, WIDE4, WIDE8, WIDE4_BYTE, WIDE4_HALF}


@pytest.mark.gpu
@pytest.mark.parametrize("which,env,form", VARIANTS, ids=variant_ids)
def test_every_execution_variant(gpu_ctx, abi, variant_reference, tree_form, monkeypatch, which, env, form):
    """samples, film and serial film byte-equal to the default variant's: one stream, the fused kernels, unsorted shading, the tables
    in HBM, the device-built tree, and each tree form (binary in LDS and in HBM, 4-wide with full-precision, byte and half-float
    boxes, 8-wide), which the plan of the scene under the knobs is asserted to be"""
    set_knobs(monkeypatch, env)
    want = variant_reference[which]
    assert tree_form(want["flat"]) == form
    g = abi.Scene(gpu_ctx, want["flat"])
    gx, gp, film, serial, st = render_three(g, abi)
    g.close()
    print("ROUGHPLASTIC variant %s %s (tree form %d): trace %d shade %d wavefront %d" % (which, EV.variant_id(env), form, st.launches_trace, st.launches_shade, st.launches_wavefront))
    assert np.array_equal(bits(gp), bits(want["pos"])) and np.array_equal(bits(gx), bits(want["xyz"])), env
    assert np.array_equal(bits(film), bits(want["film"])), (env, float(np.abs(film - want["film"]).max()))
    assert np.array_equal(bits(serial), bits(want["serial"])), env
    assert st.samples == want["samples"]
    if env.get("MSK_FUSED") == "1":
        assert st.launches_wavefront > 0


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["lds", "hbm"])
def test_mask_of_opacity_one_is_the_roughplastic_alone(gpu_ctx, hostmirror, abi, variant_reference, monkeypatch, which):
    """`mask` of opacity 1 over the roughplastics is the roughplastics alone, to the bit: samples, film, serial film"""
    for k in DM.KNOBS:
        monkeypatch.delenv(k, raising=False)
    want = variant_reference[which]
    g = abi.Scene(gpu_ctx, variant_flat(hostmirror, which, masked=True))
    try:
        assert len(g.flat.masks) == 2
        gx, gp, film, serial, _ = render_three(g, abi)
    finally:
        g.close()
    assert np.array_equal(bits(gx), bits(want["xyz"])) and np.array_equal(bits(gp), bits(want["pos"]))
    assert np.array_equal(bits(film), bits(want["film"])) and np.array_equal(bits(serial), bits(want["serial"]))


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["lds", "hbm"])
def test_the_lens_tier_against_its_own_default(gpu_ctx, hostmirror, abi, variant_reference, monkeypatch, which):
    """The roughplastics through k_shade_gen_l / k_wavefront_l / k_wavefront_h_l: a `thinlens` of aperture 0.  Every execution variant of
    that scene gives its own default's film and samples, bit for bit (against the pinhole the film positions are the same bits; the
    samples cannot be: test_plastic_bsdf.test_the_lens_tier_at_aperture_zero says why)."""
    for k in DM.KNOBS:
        monkeypatch.delenv(k, raising=False)
    want = variant_reference[which]
    flat = variant_flat(hostmirror, which, lens=True)
    assert flat.lens is not None and flat.lens.aperture_radius == 0.0
    g = abi.Scene(gpu_ctx, flat)
    xyz, pos = g.sample_pixels(abi.render_params(spp=16, seed=5), EV.crop_pixels())
    film, st = g.render(abi.render_params(spp=8, seed=5))
    g.close()
    assert np.array_equal(bits(pos), bits(want["pos"])) and st.samples == want["samples"] and np.isfinite(film).all() and film[..., :3].max() > 0
    for env in TP.LENS_VARIANTS:
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        g = abi.Scene(gpu_ctx, flat)
        gx, gp = g.sample_pixels(abi.render_params(spp=16, seed=5), EV.crop_pixels())
        gf, gs = g.render(abi.render_params(spp=8, seed=5))
        g.close()
        for k in env:
            monkeypatch.delenv(k)
        assert np.array_equal(bits(gx), bits(xyz)) and np.array_equal(bits(gp), bits(pos)) and np.array_equal(bits(gf), bits(film)), env
        print("ROUGHPLASTIC lens variant %s %s: trace %d shade %d wavefront %d" % (which, EV.variant_id(env), gs.launches_trace, gs.launches_shade, gs.launches_wavefront))


@pytest.mark.gpu
def test_shards_and_a_crop_window(gpu_ctx, hostmirror, abi, variant_reference, monkeypatch):
    """the films of sample shards (0, 2) and (1, 2) sum to the whole film, to test_plastic_bsdf's tolerance for shards (another order of
    summation: not bits); a crop window is the whole film's rows and columns, bit for bit"""
    for k in DM.KNOBS:
        monkeypatch.delenv(k, raising=False)
    want = variant_reference["lds"]
    g = abi.Scene(gpu_ctx, want["flat"])
    half = [g.render(abi.render_params(spp=8, seed=5, sample_first=r, sample_stride=2)) for r in (0, 1)]
    g.close()
    assert half[0][1].samples == half[1][1].samples == 48 * 48 * 4
    assert np.allclose(half[0][0] + half[1][0], want["film"], rtol=2e-6, atol=1e-6)
    assert not np.array_equal(bits(half[0][0]), bits(half[1][0]))
    crop = (5, 3, 24, 18)                                                # test_mask_bsdf's window
    g = abi.Scene(gpu_ctx, variant_flat(hostmirror, "lds", crop=crop))
    window, _ = g.render(abi.render_params(spp=8, seed=5))
    g.close()
    assert window.shape == (18, 24, 5) and window[..., :3].max() > 0
    assert np.array_equal(bits(window), bits(want["film"][3:21, 5:29]))


# ===================================================================================================== GPU 4, 5: aov, refusals
@pytest.mark.gpu
def test_aov_sees_a_roughplastic_surface_as_a_surface(gpu_ctx, hostmirror, abi):
    """an "aov" render of the roughplastic plane: the primary-hit channels are those of the same plane with a diffuse BSDF, bit for bit;
    the nested path integrator's RGB record is filled"""
    def flat(bsdf):
        m = DM.plane(hostmirror, bsdf)
        m.texcoords = TP.UV_QUAD
        return hostmirror.flatten([m], W48, W48, camera=CAM, env=SKY)
    g0, g = abi.Scene(gpu_ctx, flat({"type": "diffuse", "twosided": True})), abi.Scene(gpu_ctx, flat(roughplastic(0.5, 0.7, 1.4896, True, 0.3, twosided=True)))
    try:
        prm = abi.render_params(spp=4, seed=3, max_depth=3)
        types = [abi.MSK_AOV_DEPTH, abi.MSK_AOV_POSITION, abi.MSK_AOV_UV, abi.MSK_AOV_GEO_NORMAL, abi.MSK_AOV_SH_NORMAL]
        film, st = g.render_aov(prm, types)
        ref, st0 = g0.render_aov(prm, types)
        assert film.shape == ref.shape == (W48, W48, 5 + 12) and st.samples == st0.samples
        assert np.array_equal(bits(film[..., 3:]), bits(ref[..., 3:])) and np.abs(ref[..., 5:]).max() > 0
        rgba, _ = g.render_aov(prm, types + [abi.MSK_AOV_PATH_RGBA])
        assert np.array_equal(bits(rgba[..., 3:17]), bits(film[..., 3:17])) and np.isfinite(rgba).all()
        assert rgba[CROP[1]:CROP[1] + 8, CROP[0]:CROP[0] + 8, 17:20].min() > 0 and rgba[CROP[1]:CROP[1] + 8, CROP[0]:CROP[0] + 8, :3].min() > 0
    finally:
        g.close(); g0.close()


@pytest.mark.gpu
def test_refusals(gpu_ctx, hostmirror, abi):
    """`direct` on a roughplastic scene: MSK_ERR_UNSUPPORTED by name; the descriptor's refusals at scene creation, unequal alphas by the
    word "anisotropic"; type 5 keeps its refusal; the probes and the constants on an entry of another type"""
    make = lambda: hostmirror.flatten([DM.plane(hostmirror, roughplastic()), hostmirror.MeshSpec("lamp", [tuple(DM.LAMP)], hostmirror.LUMINAIRE, radiance=(40, 30, 20))], W48, W48, camera=CAM)
    g = abi.Scene(gpu_ctx, make())
    try:
        prm = abi.render_params(spp=2, seed=1)
        for call in (lambda: g.render_direct(prm, 1, 1), lambda: g.sample_pixels_direct(prm, EV.crop_pixels()[:2], 1, 1)):
            with pytest.raises(abi.MskError) as e:
                call()
            assert e.value.code == abi.MSK_ERR_UNSUPPORTED and "`roughplastic`" in str(e.value) and "direct" in str(e.value)
        film, _ = g.render(prm)                                          # (`path` renders it)
        assert film[..., :3].max() > 0
        one = np.ones((1, 3), F)
        for call in (lambda: g.roughplastic_eval(1, one[:, :2], one, one, np.full((1, 4), 550, F)), lambda: g.roughplastic_sample(1, one[:, :2], one, one, np.full((1, 4), 550, F))):
            with pytest.raises(abi.MskError) as e:
                call()
            assert e.value.code == abi.MSK_ERR_INVALID_ARG and "not a roughplastic of this scene" in str(e.value)
        for call in (lambda: g.plastic_constants(1), lambda: g.plastic_constants(7), lambda: g.plastic_eval(0, one[:, :2], one, one, np.full((1, 4), 550, F))):
            with pytest.raises(abi.MskError) as e:
                call()
            assert e.value.code == abi.MSK_ERR_INVALID_ARG and "not a plastic of this scene" in str(e.value)
        assert 0 < g.plastic_constants(0)[0] < 1
    finally:
        g.close()
    for field, value, words, code in (("ior_eta", 0.99, "roughplastic: the relative index of refraction ior_eta", abi.MSK_ERR_INVALID_ARG),
                                      ("ior_inv_eta", 0.0, "roughplastic: ior_inv_eta", abi.MSK_ERR_INVALID_ARG),
                                      ("alpha_v", 0.25, "anisotropic", abi.MSK_ERR_INVALID_ARG), ("alpha_u", float("nan"), "finite and non-negative", abi.MSK_ERR_INVALID_ARG),
                                      ("alpha_u", -0.3, "finite and non-negative", abi.MSK_ERR_INVALID_ARG),
                                      ("type", 5, "type 5 is not supported by this back end (diffuse, roughconductor, roughdielectric, dielectric, conductor)", abi.MSK_ERR_UNSUPPORTED)):
        flat = make()
        setattr(flat.desc.bsdfs[0], field, value)
        with pytest.raises(abi.MskError) as e:
            abi.Scene(gpu_ctx, flat)
        assert e.value.code == code and words in str(e.value) and "bsdf 0" in str(e.value), (field, str(e.value))
