"""The smooth `plastic` BSDF (include/msk_gpu.h at MSK_BSDF_PLASTIC): a delta dielectric coat over a diffuse base, in the mask family.

The device is held in three ways: to the fp32 restatement (plastic_ref.py) bit for bit through the probes, given the two constants
the packer computed (which are themselves held to float64); to float64 closed forms through renders; and to itself across every
execution variant, under an opacity-1 mask, and across sample shards.

CPU: the restatement checks itself; the packer, its refusals and the plan as a stand-alone native program (also under
AddressSanitizer / UBSan); the two flatteners; exports and struct layouts; the closed forms' own convergence.
GPU: probes; closed forms (counter RNG through msk_gpu_sample_pixels, and (a), (c) once more through a 32 x 32 film under
MSK_RNG_PCG_BLOCK); identities; an "aov" render; refusals, `direct` among them (it needs a scene, so it is a GPU test)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bitmap_ref as BR
import delta_ref as D
import light_ref as L
import plastic_ref as P
import radiometry_ref as R
import test_delta_light_mirror as DM
import test_envmap as EV
import test_launch_plan as LP
import test_spot_directional as SD
import test_table_placement as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
CAM, W48, CROP = EV.PLANE_CAMERA, EV.W48, EV.CROP
STEEP = dict(CAM, origin=(0, 8, 3))                                      # cos_i about 0.94 over the crop; CAM's is about 0.35
GRAZING = dict(CAM, origin=(0, 0.8, 8))                                  # ... and about 0.15
SKY = DM.SKY
bits = DM.bits
UV_QUAD = [((0, 0), (1, 0), (1, 1), (0, 1))]
ETAS = (1.0, 1.4896, 1.9)


def plastic(rho=0.5, s=1.0, eta=1.4896, nonlinear=False, **kw):
    return dict({"type": "plastic", "diffuse_reflectance": rho, "specular_reflectance": s, "int_ior": eta, "ext_ior": 1.0, "nonlinear": nonlinear}, **kw)


# ===================================================================================================== CPU: the restatement
def test_restatement_checks_itself():
    """sampling reproduces eval on the diffuse lobe (fp32, value * pdf against eval at the sampled direction, 1e-6 relative); the
    estimator's mean meets the albedo F_i s + (1 - F_i) D (1 - fdr_int) in float64; fdr_int by a direct quadrature from the inside,
    the kink substituted away, meets the identity to 1e-12; the fp32 Fresnel term against float64"""
    rng = np.random.RandomState(2)
    n = 4096
    wi = rng.normal(size=(n, 3))
    wi[:, 2] = np.abs(wi[:, 2]) + 1e-3
    wi = (wi / np.linalg.norm(wi, axis=1, keepdims=True)).astype(F)
    z = np.sqrt(rng.uniform(0, 1, n))
    phi = rng.uniform(0, 2 * np.pi, n)
    hemi = np.stack([np.sqrt(1 - z * z) * np.cos(phi), np.sqrt(1 - z * z) * np.sin(phi), z], -1).astype(F)
    rho, s = rng.uniform(0, 1, (n, 4)).astype(F), rng.uniform(0, 1, (n, 4)).astype(F)
    for eta in (1.0, 1.2, 1.4896, 1.9):
        fdr = F(P.fdr_int64(eta))
        assert abs(P.fdr_int_direct64(eta) - P.fdr_int64(eta)) <= 1e-12, (eta, P.fdr_int_direct64(eta), P.fdr_int64(eta))
        c = np.linspace(1e-4, 1, 513)
        assert np.all(np.abs(P.fresnel32(c.astype(F), eta) - P.fresnel64(c.astype(F).astype(np.float64), float(F(eta)))) <= 2e-6)
        for nonlinear in (False, True):
            for ssw in (0.0, 0.3, 1.0 - 2.0 ** -20):
                got = P.sample32(wi, np.ones(n, F), hemi, rho, s, eta, F(1) / F(eta), fdr, ssw, nonlinear)      # sample1 = 1: the diffuse lobe
                ev, pdf = P.eval32(wi, hemi, rho, eta, F(1) / F(eta), fdr, ssw, nonlinear)
                assert got["ok"].all() and not got["delta"].any() and np.array_equal(bits(got["pdf"]), bits(pdf))
                live = pdf > 0                                           # (pd = 1 - ps rounds to 0 at grazing wi under an ssw next to 1: the value is then 0)
                assert (live.all() if ssw < 0.5 else live.mean() > 0.9) and not got["value"][~live].any()
                back = got["value"].astype(np.float64) * got["pdf"][:, None]
                assert np.all(np.abs(back - ev)[live] <= 1e-6 * ev[live] + 1e-30), float(np.abs(back / np.maximum(ev, 1e-30) - 1)[live].max())
                coat = P.sample32(wi, np.zeros(n, F), hemi, rho, s, eta, F(1) / F(eta), fdr, max(ssw, 0.3), nonlinear)       # sample1 = 0 < ps
                if eta > 1:
                    assert coat["delta"].all() and np.array_equal(coat["wo"], wi * np.array([-1, -1, 1], F))
                    f_i = P.fresnel64(wi[:, 2].astype(np.float64), float(F(eta)))
                    assert np.allclose(coat["value"].astype(np.float64) * coat["pdf"][:, None], s * f_i[:, None], rtol=2e-5, atol=1e-9)
                else:
                    assert not coat["delta"].any()                       # eta = 1: F_i = 0, the coat is never sampled
            for cos_i in (0.05, 0.35, 0.9, 1.0):
                for r0, s0, w in ((0.5, 0.7, 0.4), (1.0, 1.0, 0.5), (0.0, 0.7, 1.0), (0.9, 0.0, 0.0)):
                    mean, want = P.estimator_mean64(cos_i, r0, s0, eta, w, nonlinear), float(P.albedo64(cos_i, r0, s0, eta, nonlinear))
                    assert abs(mean - want) <= 1e-9, (eta, nonlinear, cos_i, r0, s0, mean, want)
        assert abs(float(P.albedo64(0.3, 1.0, 1.0, eta, True)) - 1.0) <= 1e-12       # the white furnace: nothing is lost
    # the failures: cos_i <= 0, and ps + pd == 0
    bad = P.sample32(np.array([[0, 0.6, -0.8], [1, 0, 0]], F), np.array([0.5, 0.5], F), hemi[:2], rho[:2], s[:2], 1.5, F(1) / F(1.5), F(0.6), 0.5, False)
    assert not bad["ok"].any() and not bad["value"].any() and not bad["pdf"].any()
    none = P.sample32(wi[:4], np.full(4, 0.5, F), hemi[:4], rho[:4], s[:4], 1.0, 1.0, 0.0, 1.0, False)          # eta = 1 and ssw = 1: F_i ssw = 0 = (1 - F_i)(1 - ssw)
    assert not none["ok"].any()


# ===================================================================================================== CPU: native, layout, hosts
@pytest.fixture(scope="module")
def native_exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("plastic_tables")
    src = os.path.join(ROOT, "tests", "native", "plastic_tables_check.cpp")
    plain, san = str(d / "plastic_tables_check"), str(d / "plastic_tables_check_san")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", plain, src])
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", san, src])
    return plain, san


def test_native_packer_check(native_exe):
    """every refusal, fdr_int and ssw against float64, a scene without a plastic packing to its recorded bytes, the opacity-1 mask
    records: plain and sanitized"""
    for exe in native_exe:
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stdout.split()[0] == "ok", r.stdout[-2000:] + r.stderr[-2000:]


@pytest.mark.parametrize("knobs", LP.KNOB_SETS, ids=lambda k: ",".join(f"{a}={b}" for a, b in k.items()) or "defaults")
def test_plan_with_a_plastic(native_exe, knobs):
    """has_plastic plans what has_mask plans, field for field: SHADE_MASK, or SHADE_LENS with a lens"""
    env = {k: v for k, v in os.environ.items() if not k.startswith("MSK_")}
    env.update(knobs)
    r = subprocess.run([native_exe[0], "plan"], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    assert r.stdout.split() == ["cases", str(7 * 512 * 4 * len(LP.REGION_SIZES) * len(LP.LDS))]


def test_exports_and_struct_layouts(abi, tmp_path):
    src = tmp_path / "off.c"
    names = ("type", "back_bsdf", "reflectance", "alpha_u", "alpha_v", "sample_visible", "eta", "k", "specular_reflectance", "specular_transmittance", "ior_eta",
             "ior_inv_eta", "reflectance_texture", "reflectance_scale", "reflectance_regular")
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "msk_gpu.h"\nint main(){printf("%zu ' + "%zu " * len(names) + '%d %d\\n",sizeof(msk_bsdf_desc),'
                   + ",".join("offsetof(msk_bsdf_desc,%s)" % n for n in names) + ',MSK_BSDF_PLASTIC,MSK_ABI_VERSION);return 0;}\n')
    exe = tmp_path / "off"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    b = abi.BsdfDesc
    assert got == [C.sizeof(b)] + [getattr(b, n).offset for n in names] + [abi.MSK_BSDF_PLASTIC, abi.MSK_ABI_VERSION]
    assert got[0] == 132 and got[-2:] == [6, 8]                          # the descriptor keeps its size; type 5 stays unassigned
    import __graft_entry__ as ge
    ge.build_gpu_library()
    lib = C.CDLL(abi.LIB_PATH)
    for name in ("msk_gpu_plastic_sample", "msk_gpu_plastic_eval", "msk_gpu_plastic_constants"):
        assert name in abi.EXPORTS and getattr(lib, name) is not None


def quad(hm, name, bsdf, y=0.0, size=1.0, uv=False):
    s = float(size)
    return hm.MeshSpec(name, [((-s, y, s), (s, y, s), (s, y, -s), (-s, y, -s))], (0.6, 0.5, 0.4), bsdf=bsdf, texcoords=UV_QUAD if uv else None)


BITMAP = {"type": "bitmap", "pixels": np.random.RandomState(8).uniform(0.1, 0.9, (2, 3, 3)).astype(F), "scale": (2, 3)}
CHECKER = {"type": "checkerboard", "color0": (0.8, 0.2, 0.1), "color1": (0.1, 0.3, 0.7), "scale": (4, 4)}


def flattener_meshes(hm):
    return [quad(hm, "defaults", {"type": "plastic"}, 0.0),
            quad(hm, "twosided", plastic((0.2, 0.5, 0.7), (0.9, 0.8, 0.6), 1.9, True, twosided=True), 0.1),
            quad(hm, "masked", {"type": "mask", "opacity": 0.375, "bsdf": plastic(0.25, 0.5, 1.2, twosided=True)}, 0.2),
            quad(hm, "bitmap", plastic(dict(BITMAP), 0.7, nonlinear=True), 0.3, uv=True),
            quad(hm, "checker", plastic(dict(CHECKER), (0.5, 0.5, 0.5)), 0.4, uv=True),
            quad(hm, "iors", {"type": "plastic", "int_ior": 1.33, "ext_ior": 1.1, "specular_reflectance": 2.0}, 0.5)]


def test_the_two_flatteners_agree(hostmirror, abi, tmp_path):
    """XML through the C++ host against the dict through the Python mirror: the defaults, `twosided`, `mask` over plastic, a bitmap
    and a checkerboard diffuse reflectance: the same descriptors byte for byte; the refusal of a textured specular_reflectance in
    the same words"""
    hostlib = EV.host_library()
    xml = hostmirror.write_scene_xml(flattener_meshes(hostmirror), str(tmp_path / "s"), 16, 16, 1, camera=CAM)
    text = open(xml).read()
    assert text.count('<bsdf type="plastic">') == 6 and text.count('<bsdf type="twosided">') == 2 and text.count('<bsdf type="mask">') == 1
    h = hostlib.HostScene(xml).flatten()
    m = hostmirror.flatten(flattener_meshes(hostmirror), 16, 16, camera=CAM, coeff_lookup=hostlib.srgb_model_fetch)
    assert h.desc.n_bsdfs == m.desc.n_bsdfs == 6 and h.desc.n_textures == m.desc.n_textures == 2
    for i in range(6):
        assert bytes(h.desc.bsdfs[i]) == bytes(m.desc.bsdfs[i]), i
        assert m.desc.bsdfs[i].type == abi.MSK_BSDF_PLASTIC
    for i in range(2):
        assert bytes(h.desc.textures[i]) == bytes(m.desc.textures[i]), i
    assert h.desc.n_texels == m.desc.n_texels == 6
    assert np.array_equal(bits(np.ctypeslib.as_array(h.desc.texels, (18,))), bits(np.ctypeslib.as_array(m.desc.texels, (18,))))
    assert len(h.masks) == len(m.masks) == 1 and h.masks[0].bsdf == m.masks[0].bsdf == 2 and h.masks[0].opacity == m.masks[0].opacity == 0.375
    d = m.desc.bsdfs
    assert (d[0].reflectance_scale, d[0].specular_reflectance.scale, d[0].sample_visible, d[0].back_bsdf) == (0.5, 1.0, 0, -1)
    assert list(d[0].reflectance) == [0.0, 0.0, float("inf")] and list(d[0].specular_reflectance.coeff) == [0.0, 0.0, float("inf")]
    assert d[0].ior_eta == F(1.49) / F(1.00028) and d[0].ior_inv_eta == F(1.00028) / F(1.49)
    assert (d[1].back_bsdf, d[1].sample_visible, d[2].back_bsdf) == (1, 1, 2) and d[1].ior_eta == F(1.9)
    assert (d[3].reflectance_texture, d[4].reflectance_texture, d[3].sample_visible) == (1, 2, 1)
    assert d[5].ior_eta == F(1.33) / F(1.1) and d[5].specular_reflectance.scale == 2.0
    # the refusal, worded alike
    tex = '<texture name="specular_reflectance" type="checkerboard"><rgb name="color0" value="0.1"/><rgb name="color1" value="0.2"/></texture>'
    plain = hostmirror.write_scene_xml([quad(hostmirror, "q", None)], str(tmp_path / "r"), 16, 16, 1, camera=CAM)
    text = open(plain).read()
    start, end = text.index("<bsdf"), text.index("</bsdf>") + len("</bsdf>")
    path = tmp_path / "r" / "bad.xml"
    path.write_text(text[:start] + '<bsdf type="plastic">' + tex + '</bsdf>' + text[end:])
    with pytest.raises(hostlib.HostError) as e:
        hostlib.HostScene(str(path)).flatten()
    assert hostmirror.PLASTIC_SPECULAR in str(e.value), str(e.value)
    with pytest.raises(ValueError) as e:
        hostmirror.flatten([quad(hostmirror, "q", plastic(0.5, dict(CHECKER)))], 16, 16, camera=CAM)
    assert hostmirror.PLASTIC_SPECULAR in str(e.value)
    assert "conductor" not in hostmirror.PLASTIC_SPECULAR and hostmirror.PLASTIC_SPECULAR.endswith("(a texture that varies over the surface is not supported)")


# ===================================================================================================== float64 expectations
def sky_xyz(desc, e=0):
    return R.expected_xyz(D.emitter_spectrum(desc, e), DM.cie_of(desc))


def crop_cosines(desc, m):
    o, d, w = DM.crop_rays(desc, m)
    x = R.hit_plane(o, d, (0, 0, 0), (0, 1, 0))
    assert np.all(np.abs(x[..., [0, 2]]) < 50)
    return -d[..., 1], w, o, d, x


LAMP_WALL = [(-30.0, 0.0, DM.WALL_Z), (30.0, 0.0, DM.WALL_Z), (30.0, 30.0, DM.WALL_Z), (-30.0, 30.0, DM.WALL_Z)]          # faces +z, as DM's wall


def grey_value(desc, m, rho, s, nonlinear):
    c, w = crop_cosines(desc, m)[:2]
    return float((w * P.albedo64(c, rho, s, float(desc.bsdfs[0].ior_eta), nonlinear)).sum())


def sun_value(flat, c_view, nonlinear, rho):
    """E_sun cos_s D / pi / eta^2 (1 - F_s)(1 - F_view) per unit of the sun's irradiance spectrum"""
    eta = float(flat.desc.bsdfs[0].ior_eta)
    cos_s = L.sun_geometry((0, 1, 0), SD.light_of(flat, 0)[1])
    return P.eval64(cos_s, c_view, rho, eta, nonlinear) / c_view * cos_s


def mirror_value(desc, m, s):
    c, w, o, d, x0 = crop_cosines(desc, m)
    d1 = D.reflect(d, (0, 1, 0))
    t = (DM.WALL_Z - x0[..., 2]) / d1[..., 2]
    x1 = x0 + d1 * t[..., None]
    assert np.all(t > 0) and np.all(x1[..., 1] > 1) and np.all(x1[..., 1] < 29) and np.all(np.abs(x1[..., 0]) < 29)      # every mirrored ray meets the lamp's interior
    return float((w * P.fresnel64(c, float(desc.bsdfs[0].ior_eta)) * s).sum())


def closed_form_case(hm, name):
    """-> (flat, expectation at 4 x 4 nodes over the crop, the same at 8 x 8, render parameters)"""
    kind = name.split("_")[0]
    if kind == "a":                                                      # the white furnace: exactly the sky, at any view
        cam = STEEP if name.endswith("steep") else GRAZING
        flat = hm.flatten([DM.plane(hm, plastic(1.0, 1.0, 1.4896, True))], W48, W48, camera=cam, env=SKY)
        c = crop_cosines(flat.desc, 4)[0]
        assert (c.min() > 0.9) if cam is STEEP else (c.max() < 0.2)
        return flat, sky_xyz(flat.desc), sky_xyz(flat.desc), dict(max_depth=2)
    if kind == "b":
        nonlinear, eta = "nonlinear" in name, 1.9 if name.endswith("19") else 1.4896
        flat = hm.flatten([DM.plane(hm, plastic(0.5, 0.7, eta, nonlinear))], W48, W48, camera=CAM, env=SKY)
        return (flat, *(sky_xyz(flat.desc) * grey_value(flat.desc, m, 0.5, 0.7, nonlinear) for m in (4, 8)), dict(max_depth=2))
    if kind == "c":
        flat = hm.flatten([DM.plane(hm, plastic(0.5, 0.7, 1.4896, True))], W48, W48, camera=CAM, lights=[SD.sun_spec()])
        out = []
        for m in (4, 8):
            c, w = crop_cosines(flat.desc, m)[:2]
            out.append(sky_xyz(flat.desc) * float((w * sun_value(flat, c, True, 0.5)).sum()))
        return flat, out[0], out[1], dict(max_depth=2)
    if kind == "d":
        lamp = hm.MeshSpec("lamp", [tuple(LAMP_WALL)], hm.LUMINAIRE, radiance=(40, 30, 20))
        flat = hm.flatten([DM.plane(hm, plastic(0.0, 0.7, 1.4896)), lamp], W48, W48, camera=CAM)
        return (flat, *(sky_xyz(flat.desc) * mirror_value(flat.desc, m, 0.7) for m in (4, 8)), dict(max_depth=2))
    raise KeyError(name)


CASES = ["a_furnace_steep", "a_furnace_grazing", "b_grey_linear_149", "b_grey_nonlinear_149", "b_grey_linear_19", "b_grey_nonlinear_19", "c_sun", "d_black_base_mirrors_a_lamp"]


@pytest.mark.parametrize("name", CASES)
def test_expectations_have_converged(hostmirror, name):
    """the 4 x 4 Gauss-Legendre rule over the crop against 8 x 8, and the wavelength quadrature of expected_xyz at 16 against 32 nodes"""
    flat, e4, e8, _ = closed_form_case(hostmirror, name)
    print("PLASTIC %s: expectation %s (8 x 8 nodes: %s)" % (name, e4, e8))
    assert np.all(e4 > 0) and np.all(np.abs(e4 - e8) <= 1e-5 * e8)
    s = D.emitter_spectrum(flat.desc, 0)
    assert np.all(np.abs(R.expected_xyz(s, DM.cie_of(flat.desc), 16) - R.expected_xyz(s, DM.cie_of(flat.desc), 32)) <= 1e-5 * R.expected_xyz(s, DM.cie_of(flat.desc), 32))


def film_case(hm, name, m=10):
    """(a), (c) on DM.film_case's 32 x 32 film: (flat, expectation of sum XYZ / sum W, effective samples / samples)"""
    if name == "a":
        flat = hm.flatten([DM.plane(hm, plastic(1.0, 1.0, 1.4896, True))], 32, 32, camera=CAM, env=SKY)
        value = lambda o, d: np.ones(d.shape[:-1])
    else:
        flat = hm.flatten([DM.plane(hm, plastic(0.5, 0.7, 1.4896, True))], 32, 32, camera=CAM, lights=[SD.sun_spec()])
        value = lambda o, d: sun_value(flat, -d[..., 1], True, 0.5)
    t, a, n_eff = DM.film_weights(flat.desc, 32, m)
    yy, xx = np.meshgrid(t, t, indexing="ij")
    o, d = R.camera_ray(flat.desc, xx, yy)
    return flat, sky_xyz(flat.desc) * float(np.einsum("j,k,jk->", a, a, value(o, d))), n_eff


@pytest.mark.parametrize("name", ["a", "c"])
def test_film_expectations_have_converged(hostmirror, name):
    _, fine, n_eff = film_case(hostmirror, name, 14)
    _, coarse, _ = film_case(hostmirror, name, 10)
    print("PLASTIC film %s: fine %s coarse %s effective samples / samples %.4f" % (name, fine, coarse, n_eff))
    assert np.all(np.abs(coarse - fine) <= 1e-5 * fine) and 0.8 < n_eff < 1.0


# ===================================================================================================== GPU 1: the probes
def probe_entries():
    """(name, spec): eta 1, 1.4896 and 1.9; both `nonlinear`; ssw of 1 (a black base), near 0 (a faint coat) and in between; a bitmap
    and a checkerboard rho; one-sided and twosided"""
    out = []
    for eta in ETAS:
        out.append(("grey_%g" % eta, plastic((0.6, 0.5, 0.4), (0.9, 0.8, 0.7), eta, False)))
        out.append(("nonlinear_%g" % eta, plastic((0.9, 0.95, 0.99), 0.7, eta, True, twosided=True)))
    out += [("black_base", plastic(0.0, 0.7, 1.4896, True)), ("faint_coat", plastic(0.9, 1e-6, 1.4896, False, twosided=True)), ("no_coat", plastic(0.5, 0.0, 1.9, True)),
            ("bitmap", plastic(dict(BITMAP), 0.7, 1.4896, True)), ("checker", plastic(dict(CHECKER), (0.5, 0.6, 0.7), 1.9, False, twosided=True))]
    return out


def probe_inputs(rng, n, ps_of):
    uv = rng.uniform(-1.5, 1.5, (n, 2)).astype(F)
    wi = rng.normal(size=(n, 3))
    wi = (wi / np.linalg.norm(wi, axis=1, keepdims=True)).astype(F)
    wi[0::16] = [0, 0, 1]
    wi[1::16] = [1, 0, 0]                                                # cos_i = 0
    wi[2::16, 2] = -np.abs(wi[2::16, 2])                                 # a negative cos_i
    z = F(1e-4)
    wi[3::16] = [np.sqrt(F(1) - z * z), 0, z]                            # cos_i = 1e-4
    wo = rng.normal(size=(n, 3))
    wo = (wo / np.linalg.norm(wo, axis=1, keepdims=True)).astype(F)
    wo[4::16] = [0, 1, 0]
    su = rng.uniform(0, 1, (n, 3)).astype(F)
    ps = ps_of(wi)                                                       # sample1 on both sides of ps and equal to it
    su[5::8, 0], su[6::8, 0], su[7::8, 0] = ps[5::8], np.nextafter(ps[6::8], F(-1)), np.nextafter(ps[7::8], F(2))
    su[:, 0] = np.clip(np.nan_to_num(su[:, 0], nan=0.5), 0, np.nextafter(F(1), F(0)))
    wl = rng.uniform(360, 830, (n, 4)).astype(F)
    return uv, wi, wo, su, wl


def rho32(oracle, flat, b, uv, wl):
    """the diffuse reflectance of entry b at uv and wl, float32 [n, 4]: the constant, a checkerboard colour or the bitmap lookup"""
    d = flat.desc
    bd = d.bsdfs[b]
    if bd.reflectance_texture == 0:
        return (D.sigmoid32(oracle if not np.isinf(bd.reflectance[2]) else None, bd.reflectance[:], wl) * F(bd.reflectance_scale)).astype(F)
    td = d.textures[bd.reflectance_texture - 1]
    if td.type == 1:
        fu, fv = BR.frac_uv(list(td.to_uv), uv)
        first = (fu > F(0.5)) == (fv > F(0.5))
        return np.where(first[:, None], D.sigmoid32(oracle, td.color0[:], wl), D.sigmoid32(oracle, td.color1[:], wl)).astype(F)
    coeffs = flat.texels[td.first_texel:td.first_texel + td.width * td.height].reshape(td.height, td.width, 3)
    return BR.lookup(BR.oracle_texels(oracle, coeffs), td.width, td.height, "bilinear", list(td.to_uv), uv, wl)


@pytest.mark.gpu
@pytest.mark.parametrize("tables", ["lds", "hbm"])
def test_probes_equal_the_restatement_bit_for_bit(gpu_ctx, oracle, hostmirror, abi, tables):
    """(1) msk_gpu_plastic_sample / msk_gpu_plastic_eval against plastic_ref, given the constants msk_gpu_plastic_constants returns, which are
    held to float64 here: fdr_int to 2e-7 relative, ssw to 1e-6.  11 entries x 256 inputs; `hbm`: the same scene padded until its
    small tables no longer fit LDS (the probes read them from memory either way; the renders of this scene are what differ)"""
    entries = probe_entries()
    meshes = [quad(hostmirror, name, spec, 0.1 * i, uv=True) for i, (name, spec) in enumerate(entries)]
    meshes.append(hostmirror.MeshSpec("lamp", [tuple(DM.LAMP)], hostmirror.LUMINAIRE, radiance=(40, 30, 20)))
    flat = hostmirror.flatten(meshes, 16, 16, camera=CAM, coeff_lookup=None)
    if tables == "hbm":
        pads = T.faceless_pads(hostmirror, T.SMALL_TABLES_F4 + 1 - T.table_plan(flat)["small_f4"])
        flat = hostmirror.flatten(meshes + pads, 16, 16, camera=CAM, coeff_lookup=None)
        assert T.table_plan(flat)["small_f4"] > T.SMALL_TABLES_F4
    g = abi.Scene(gpu_ctx, flat)
    rng = np.random.RandomState(11)
    try:
        for b, (name, spec) in enumerate(entries):
            bd = flat.desc.bsdfs[b]
            fdr, ssw = g.plastic_constants(b)
            eta, inv_eta, nonlinear = F(bd.ior_eta), F(bd.ior_inv_eta), bool(bd.sample_visible)
            want_fdr, want_ssw = P.fdr_int64(float(eta)), P.desc_ssw64(flat.desc, b, flat.texels)
            assert abs(float(fdr) - want_fdr) <= 2e-7 * want_fdr and abs(float(ssw) - want_ssw) <= 1e-6, (name, fdr, want_fdr, ssw, want_ssw)
            if name == "black_base":
                assert ssw == 1.0
            if name == "faint_coat":
                assert 0 < ssw < 2e-6
            twosided = bd.back_bsdf >= 0

            def front(w):
                return np.where((w[:, 2:3] < 0) & twosided, w * np.array([1, 1, -1], F), w).astype(F), (w[:, 2] < 0) & twosided

            uv, wi, wo_in, su, wl = probe_inputs(rng, 256, lambda w: P.lobes32(front(w)[0][:, 2], eta, ssw)[2])
            wif, flipped = front(wi)
            rho = rho32(oracle, flat, b, uv, wl)
            s = D.spectrum32(oracle if not np.isinf(bd.specular_reflectance.coeff[2]) else None, bd.specular_reflectance, wl)
            hemi = np.array([oracle.warps(u)[2] for u in su[:, 1:]], F)
            want = P.sample32(wif, su[:, 0], hemi, rho, s, eta, inv_eta, fdr, ssw, nonlinear)
            want["wo"][flipped, 2] = -want["wo"][flipped, 2]
            wo_pdf, value, flags = g.plastic_sample(b, uv, wi, su, wl)
            assert np.array_equal(flags[:, 3] != 0, want["ok"]) and np.array_equal(flags[:, 1] != 0, want["delta"]), name
            assert not flags[:, 2].any() and np.all(flags[:, 0] == 1)     # no null lobe without a mask; eta = 1
            if float(eta) > 1 and name not in ("no_coat",):
                assert want["delta"].any() and (want["ok"] & ~want["delta"]).any() if name != "black_base" else want["delta"][want["ok"]].all()
            for what, got, ref in (("wo", wo_pdf[:, :3], want["wo"]), ("pdf", wo_pdf[:, 3], want["pdf"]), ("value", value, want["value"])):
                bad = (bits(got) != bits(ref)).reshape(len(wi), -1).any(-1) & ~((got == 0) & (ref == 0)).reshape(len(wi), -1).all(-1)
                assert not bad.any(), (tables, name, what, int(bad.sum()), got[bad][:3], ref[bad][:3], wi[bad][:3], su[bad][:3])
            a_pdf, ev = g.plastic_eval(b, uv, wi, wo_in, wl)
            wof = np.where(flipped[:, None], wo_in * np.array([1, 1, -1], F), wo_in).astype(F)
            rv, rp = P.eval32(wif, wof, rho, eta, inv_eta, fdr, ssw, nonlinear)
            assert np.all(a_pdf[:, 0] == 1)
            for what, got, ref in (("eval", ev, rv), ("eval pdf", a_pdf[:, 1], rp)):
                bad = (bits(got) != bits(ref)).reshape(len(wi), -1).any(-1)
                assert not bad.any(), (tables, name, what, int(bad.sum()), got[bad][:3], ref[bad][:3])
            assert rp.max() > 0 or name == "black_base" and ssw == 1
        with pytest.raises(abi.MskError) as err:                         # the lamp's BSDF is not a plastic
            g.plastic_sample(len(entries), uv[:1], wi[:1], su[:1], wl[:1])
        assert "not a plastic" in str(err.value) and err.value.code == abi.MSK_ERR_INVALID_ARG
        with pytest.raises(abi.MskError) as err:                         # msk_gpu_mask_sample still wants a mask
            g.mask_sample(0, uv[:1], wi[:1], su[:1], wl[:1])
        assert "holds no mask" in str(err.value)
    finally:
        g.close()


# ===================================================================================================== GPU 2: closed forms
def sampled_mean(g, abi, what, expected, **params):
    """test_mask_bsdf's procedure: spp doubles from 4096 until the standard error (from the per-sample values) is at most 0.5 % of
    the expectation, four doublings at the most"""
    spp = 4096
    for _ in range(5):
        xyz, _ = g.sample_pixels(abi.render_params(spp=spp, seed=7, **params), EV.crop_pixels())
        v = xyz.reshape(-1, 3).astype(np.float64)
        mean, se = v.mean(0), v.std(0, ddof=1) / np.sqrt(len(v))
        print("PLASTIC %s %s spp %d: expected %s mean %s se/|E| %s dev/|E| %s" % (what, params, spp, expected, mean, se / expected, (mean - expected) / expected))
        if np.all(se <= 5e-3 * expected):
            return mean, se
        spp *= 2
    raise AssertionError("the standard error stays above 0.5 %% of the expectation: %s" % (se / expected,))


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_rendered_radiance_meets_the_closed_form(gpu_ctx, hostmirror, abi, name):
    """(a) the white furnace gives the sky at a steep and at a grazing view; (b) L [F_i s + (1 - F_i) D (1 - fdr_int)]; (c) a sun on the
    plane lights the diffuse lobe alone; (d) a black base mirrors an area lamp, F(cos_i) s Le, the emitter counted with weight 1 after
    the coat's delta lobe: |mean - E| <= 6 standard errors + 1e-3 E per channel"""
    flat, expected, _, params = closed_form_case(hostmirror, name)
    g = abi.Scene(gpu_ctx, flat)
    try:
        if name.startswith("d"):
            assert g.plastic_constants(0)[1] == 1.0                      # every sample is the mirror lobe
        mean, se = sampled_mean(g, abi, name, expected, **params)
    finally:
        g.close()
    assert np.all(np.abs(mean - expected) <= 6 * se + 1e-3 * expected), ((mean - expected) / expected, se / expected)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["a", "c"])
def test_film_in_pcg_block_mode_meets_the_closed_form(gpu_ctx, hostmirror, abi, name):
    """(a), (c) under MSK_RNG_PCG_BLOCK (k_path_serial_m) through a 32 x 32 film, by the procedure of test_delta_light_mirror's film test"""
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
    print("PLASTIC film %s: expected %s mean %s se/|E| %s dev/|E| %s" % (name, expected, mean, se / expected, (mean - expected) / expected))
    assert np.all(se <= 5e-3 * expected)
    assert np.all(np.abs(mean - expected) <= 6 * se + 1e-3 * expected)


@pytest.mark.gpu
def test_one_sided_plastic_is_black_from_behind(gpu_ctx, hostmirror, abi):
    """(e) the plane wound the other way round, under the sun that lights (c): exact zeros, samples and serial film; twosided, it is lit"""
    for twosided in (False, True):
        flat = hostmirror.flatten([DM.plane(hostmirror, plastic(0.5, 0.7, 1.4896, True, twosided=twosided), flip=True)], W48, W48, camera=CAM, lights=[SD.sun_spec()])
        g = abi.Scene(gpu_ctx, flat)
        try:
            xyz, _ = g.sample_pixels(abi.render_params(spp=64, seed=7, max_depth=3), EV.crop_pixels())
            film, _ = g.render(EV.pcg(abi, spp=4, seed=7, max_depth=3))
        finally:
            g.close()
        rows = film[CROP[1]:CROP[1] + 8, CROP[0]:CROP[0] + 8, :3]
        assert (xyz.min() > 0 and rows.min() > 0) if twosided else (not xyz.any() and not rows.any())


# ===================================================================================================== GPU 3: identities
def variant_meshes(hm, pads=(), masked=False):
    """test_envmap's box (open Cornell box, area light, bitmap floor, glass ball) with plastic boxes: a nonlinear twosided one with a
    bitmap base on the tall box, a one-sided coloured one on the short box; masked: both under a mask of opacity 1"""
    meshes = EV.variant_meshes(hm, pads)
    by = {m.name: m for m in meshes}
    big, small = by["cbox_largebox"], by["cbox_smallbox"]
    big.bsdf = plastic({"type": "bitmap", "pixels": np.random.RandomState(4).uniform(0.2, 0.9, (4, 4, 3)).astype(F), "scale": (3, 2)}, 0.8, 1.4896, True, twosided=True)
    big.texcoords = [((0, 0), (1, 0), (1, 1), (0, 1)) for _ in big.faces]
    small.bsdf = plastic((0.7, 0.3, 0.2), (0.9, 0.9, 0.8), 1.9, False)
    if masked:
        big.bsdf = {"type": "mask", "opacity": 1.0, "bsdf": big.bsdf}
        small.bsdf = {"type": "mask", "opacity": 1.0, "bsdf": small.bsdf}
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


@pytest.fixture(scope="module")
def variant_reference(gpu_ctx, hostmirror, abi):
    """the default variant's samples and films of the two scenes (no knob set): computed once, never changed"""
    saved = {k: os.environ.pop(k) for k in DM.KNOBS if k in os.environ}
    out = {}
    try:
        for which in ("lds", "hbm"):
            flat = variant_flat(hostmirror, which)
            g = abi.Scene(gpu_ctx, flat)
            xyz, pos = g.sample_pixels(abi.render_params(spp=16, seed=5), EV.crop_pixels())
            film, st = g.render(abi.render_params(spp=8, seed=5))
            serial, _ = g.render(EV.pcg(abi, spp=2, seed=5))
            g.close()
            for a in (xyz, pos, film, serial):
                a.setflags(write=False)
            assert np.isfinite(film).all() and film[..., :3].max() > 0
            out[which] = dict(flat=flat, xyz=xyz, pos=pos, film=film, serial=serial, samples=st.samples)
    finally:
        os.environ.update(saved)
    return out


VARIANTS = [("lds", {"MSK_STREAMS": "1"}), ("lds", {"MSK_FUSED": "1"}), ("lds", {"MSK_SORT": "0"}), ("lds", {"MSK_LDS_SCENE_KB": "0"}),
            ("hbm", {"MSK_LDS_SCENE_KB": "0"}), ("hbm", {"MSK_LDS_SCENE_KB": "0", "MSK_FUSED": "1"}), ("hbm", {"MSK_LDS_SCENE_KB": "0", "MSK_SORT": "0", "MSK_STREAMS": "1"})]


@pytest.mark.gpu
@pytest.mark.parametrize("which,env", VARIANTS, ids=lambda v: EV.variant_id(v) if isinstance(v, dict) else str(v))
def test_every_execution_variant(gpu_ctx, abi, variant_reference, monkeypatch, which, env):
    """samples, film and serial film byte-equal to the default variant's: one stream, the fused kernels, unsorted shading, the tree
    and the tables in HBM"""
    for k in DM.KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    want = variant_reference[which]
    g = abi.Scene(gpu_ctx, want["flat"])
    gx, gp = g.sample_pixels(abi.render_params(spp=16, seed=5), EV.crop_pixels())
    film, st = g.render(abi.render_params(spp=8, seed=5))
    serial, _ = g.render(EV.pcg(abi, spp=2, seed=5))
    g.close()
    print("PLASTIC variant %s %s: trace %d shade %d wavefront %d" % (which, EV.variant_id(env), st.launches_trace, st.launches_shade, st.launches_wavefront))
    assert np.array_equal(bits(gp), bits(want["pos"])) and np.array_equal(bits(gx), bits(want["xyz"])), env
    assert np.array_equal(bits(film), bits(want["film"])), (env, float(np.abs(film - want["film"]).max()))
    assert np.array_equal(bits(serial), bits(want["serial"])), env
    assert st.samples == want["samples"]
    if env.get("MSK_FUSED") == "1":
        assert st.launches_wavefront > 0


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["lds", "hbm"])
def test_mask_of_opacity_one_is_the_plastic_alone(gpu_ctx, hostmirror, abi, variant_reference, monkeypatch, which):
    """`mask` of opacity 1 over the plastics is the plastics alone, to the bit: samples, film, serial film"""
    for k in DM.KNOBS:
        monkeypatch.delenv(k, raising=False)
    want = variant_reference[which]
    g = abi.Scene(gpu_ctx, variant_flat(hostmirror, which, masked=True))
    try:
        assert len(g.flat.masks) == 2
        gx, gp = g.sample_pixels(abi.render_params(spp=16, seed=5), EV.crop_pixels())
        film, _ = g.render(abi.render_params(spp=8, seed=5))
        serial, _ = g.render(EV.pcg(abi, spp=2, seed=5))
    finally:
        g.close()
    assert np.array_equal(bits(gx), bits(want["xyz"])) and np.array_equal(bits(gp), bits(want["pos"]))
    assert np.array_equal(bits(film), bits(want["film"])) and np.array_equal(bits(serial), bits(want["serial"]))


LENS_VARIANTS = [{"MSK_FUSED": "1"}, {"MSK_SORT": "0", "MSK_STREAMS": "1"}, {"MSK_LDS_SCENE_KB": "0"}, {"MSK_LDS_SCENE_KB": "0", "MSK_FUSED": "1"}]


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["lds", "hbm"])
def test_the_lens_tier_at_aperture_zero(gpu_ctx, hostmirror, abi, variant_reference, monkeypatch, which):
    """The plastics through k_shade_gen_l / k_wavefront_l / k_wavefront_h_l: a `thinlens` of aperture 0.  Every execution variant of
    that scene gives its default's film and samples, bit for bit.  Against the pinhole's default the film positions are the same
    bits and the samples are not: at R = 0 the lens ray (msk_lens_desc) has the pinhole's origin and a direction up to 4 units of
    2^-24 beside the pinhole's (test_thinlens.py pins both rays bit for bit), and a path's radiance follows its camera ray's direction
    smoothly except where it crosses an edge.  So the samples are held by a median, which the few edge crossings cannot move: the
    relative difference of half of the lit samples stays under 1e-5, forty times the direction's 2.4e-7 (the crop sees the boxes from
    some 1000 units away, and a lobe's value moves with the hit point over lengths of tens of units)."""
    for k in DM.KNOBS:
        monkeypatch.delenv(k, raising=False)
    want = variant_reference[which]
    flat = variant_flat(hostmirror, which, lens=True)
    assert flat.lens is not None and flat.lens.aperture_radius == 0.0
    g = abi.Scene(gpu_ctx, flat)
    xyz, pos = g.sample_pixels(abi.render_params(spp=16, seed=5), EV.crop_pixels())
    film, st = g.render(abi.render_params(spp=8, seed=5))
    with pytest.raises(abi.MskError):
        g.render(EV.pcg(abi, spp=2, seed=5))                             # MSK_RNG_PCG_BLOCK refuses a lens
    g.close()
    assert np.array_equal(bits(pos), bits(want["pos"])) and st.samples == want["samples"]
    a, b = xyz.astype(np.float64).reshape(-1, 3), want["xyz"].astype(np.float64).reshape(-1, 3)
    lit = (b > 0).all(-1)
    rel = (np.abs(a - b)[lit] / b[lit]).max(-1)
    print("PLASTIC lens %s: %d lit samples, median relative difference to the pinhole %.3g, 99th percentile %.3g" % (which, lit.sum(), np.median(rel), np.percentile(rel, 99)))
    assert lit.sum() > 500 and np.median(rel) <= 1e-5
    for env in LENS_VARIANTS:
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        g = abi.Scene(gpu_ctx, flat)
        gx, gp = g.sample_pixels(abi.render_params(spp=16, seed=5), EV.crop_pixels())
        gf, gs = g.render(abi.render_params(spp=8, seed=5))
        g.close()
        for k in env:
            monkeypatch.delenv(k)
        assert np.array_equal(bits(gx), bits(xyz)) and np.array_equal(bits(gp), bits(pos)) and np.array_equal(bits(gf), bits(film)), env
        print("PLASTIC lens variant %s %s: trace %d shade %d wavefront %d" % (which, EV.variant_id(env), gs.launches_trace, gs.launches_shade, gs.launches_wavefront))


@pytest.mark.gpu
def test_shards(gpu_ctx, abi, variant_reference, monkeypatch):
    """the films of sample shards (0, 2) and (1, 2) sum to the whole film, to test_mask_bsdf's tolerance for shards (another order of
    summation: not bits)"""
    for k in DM.KNOBS:
        monkeypatch.delenv(k, raising=False)
    want = variant_reference["lds"]
    g = abi.Scene(gpu_ctx, want["flat"])
    half = [g.render(abi.render_params(spp=8, seed=5, sample_first=r, sample_stride=2)) for r in (0, 1)]
    g.close()
    assert half[0][1].samples == half[1][1].samples == 48 * 48 * 4
    assert np.allclose(half[0][0] + half[1][0], want["film"], rtol=2e-6, atol=1e-6)
    assert not np.array_equal(bits(half[0][0]), bits(half[1][0]))


# ===================================================================================================== GPU 4: aov, refusals
@pytest.mark.gpu
def test_aov_sees_a_plastic_surface_as_a_surface(gpu_ctx, hostmirror, abi):
    """an "aov" render of the plastic plane: the primary-hit channels are those of the same plane with a diffuse BSDF, bit for bit; the
    nested path integrator's RGB record is filled"""
    def flat(bsdf):
        m = DM.plane(hostmirror, bsdf)
        m.texcoords = UV_QUAD
        return hostmirror.flatten([m], W48, W48, camera=CAM, env=SKY)
    g0, g = abi.Scene(gpu_ctx, flat({"type": "diffuse", "twosided": True})), abi.Scene(gpu_ctx, flat(plastic(0.5, 0.7, 1.4896, True, twosided=True)))
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
    """`direct` on a plastic scene: MSK_ERR_UNSUPPORTED by name; an ior_eta below 1 or not finite: MSK_ERR_INVALID_ARG by name; type 5
    keeps its refusal; the probes and the constants on an entry that is no plastic"""
    make = lambda: hostmirror.flatten([DM.plane(hostmirror, plastic()), hostmirror.MeshSpec("lamp", [tuple(DM.LAMP)], hostmirror.LUMINAIRE, radiance=(40, 30, 20))], W48, W48, camera=CAM)
    g = abi.Scene(gpu_ctx, make())
    try:
        prm = abi.render_params(spp=2, seed=1)
        for call in (lambda: g.render_direct(prm, 1, 1), lambda: g.sample_pixels_direct(prm, EV.crop_pixels()[:2], 1, 1)):
            with pytest.raises(abi.MskError) as e:
                call()
            assert e.value.code == abi.MSK_ERR_UNSUPPORTED and "plastic" in str(e.value) and "direct" in str(e.value)
        film, _ = g.render(prm)                                          # (`path` renders it)
        assert film[..., :3].max() > 0
        one = np.ones((1, 3), F)
        for call in (lambda: g.plastic_constants(1), lambda: g.plastic_eval(1, one[:, :2], one, one, np.full((1, 4), 550, F)), lambda: g.plastic_constants(7)):
            with pytest.raises(abi.MskError) as e:
                call()
            assert e.value.code == abi.MSK_ERR_INVALID_ARG and "not a plastic" in str(e.value)
    finally:
        g.close()
    for field, value, words, code in (("ior_eta", 0.99, "ior_eta", abi.MSK_ERR_INVALID_ARG), ("ior_eta", float("nan"), "ior_eta", abi.MSK_ERR_INVALID_ARG),
                                      ("ior_eta", float("inf"), "ior_eta", abi.MSK_ERR_INVALID_ARG), ("ior_inv_eta", 0.0, "ior_inv_eta", abi.MSK_ERR_INVALID_ARG),
                                      ("type", 5, "type 5 is not supported by this back end (diffuse, roughconductor, roughdielectric, dielectric, conductor)", abi.MSK_ERR_UNSUPPORTED)):
        flat = make()
        setattr(flat.desc.bsdfs[0], field, value)
        with pytest.raises(abi.MskError) as e:
            abi.Scene(gpu_ctx, flat)
        assert e.value.code == code and words in str(e.value) and "bsdf 0" in str(e.value), (field, str(e.value))
