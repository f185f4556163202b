"""The smooth `dielectric` BSDF (bsdfs/dielectric.cpp): glass.

The CPU oracle renders it too (oracle.cpp: dielectric_sample), and tests/test_dielectric_parity.py compares the device with that
twin bit for bit, and the twin with float64 through the helpers of this module.  What this module pins needs no twin:

  * identities that need no oracle.  Behind one interface in a constant environment a sample's value is the environment's
    times ONE of two exactly known factors (the reflection weight or the transmission weight eta_ti^2), so the ratio of a
    sample's XYZ to the XYZ of the same (pixel, sample index, seed) in a companion scene without the glass is one of a few
    numbers, and how often each occurs is a binomial count whose mean is the float64 Fresnel term (tests/dielectric_ref.py);
  * films that are byte-identical across the library's execution variants, and to the film of the scene without the glass
    when no ray can reach it;
  * float64 closed forms (a lossless slab returns the environment's radiance, with and without Russian roulette).

Rounding bound of a ratio (set by the issue that introduced the BSDF): 16 * 2^-24 * (1 + interface events), relative.  The
factor of a path multiplies the four non-negative terms of spectrum_to_xyz's sum alike, so nothing cancels.  The binomial
checks hold |count - sum R| <= 5 sqrt(sum R (1 - R)) + 1 with R evaluated in float64 at every sample's own film position.
"""
import ctypes as C

import numpy as np
import pytest

import dielectric_ref as D
import radiometry_ref as R

EPS = 16.0 * 2.0 ** -24
ETA = 1.5
F32 = np.float32
GLASS = {"type": "dielectric", "int_ior": 1.5, "ext_ior": 1.0, "specular_reflectance": 1.0, "specular_transmittance": 1.0}
NO_RR = dict(max_depth=-1, rr_depth=1000)


def quad(c, u, v):
    """A quad centred at c spanned by +-u, +-v; its front faces u x v"""
    c, u, v = (np.asarray(a, np.float64) for a in (c, u, v))
    return tuple(tuple(float(x) for x in p) for p in (c - u - v, c + u - v, c + u + v, c - u + v))


def up_quad(y, half):
    return quad((0, y, 0), (0, 0, half), (half, 0, 0))          # z x x = +y


def down_quad(y, half):
    return quad((0, y, 0), (half, 0, 0), (0, 0, half))          # x x z = -y


def box(c, h):
    """Six outward-facing quads of the box c +- h"""
    c, (hx, hy, hz) = np.asarray(c, np.float64), h
    return [quad(c + (hx, 0, 0), (0, hy, 0), (0, 0, hz)), quad(c - (hx, 0, 0), (0, 0, hz), (0, hy, 0)),
            quad(c + (0, hy, 0), (0, 0, hz), (hx, 0, 0)), quad(c - (0, hy, 0), (hx, 0, 0), (0, 0, hz)),
            quad(c + (0, 0, hz), (hx, 0, 0), (0, hy, 0)), quad(c - (0, 0, hz), (0, hy, 0), (hx, 0, 0))]


def tables(desc):
    return np.ctypeslib.as_array(desc.cie1931_xyz, (3 * R.CIE_SAMPLES,)).astype(np.float64)


# ============================================================================= CPU: the host side and the float64 reference
@pytest.fixture(scope="module")
def hostlib():
    import importlib
    import __graft_entry__ as ge
    ge.build_gpu_library()
    ge.build_host_library()
    return importlib.import_module("misaki-render_amd.hostlib")


DESC_CASES = {
    "defaults": {"type": "dielectric"},
    "explicit_iors": {"type": "dielectric", "int_ior": 1.33, "ext_ior": 1.0},
    "dense_outside": {"type": "dielectric", "int_ior": 1.0, "ext_ior": 1.5},
    "tinted_rgb": {"type": "dielectric", "int_ior": 1.5046, "specular_reflectance": (0.9, 0.5, 0.2), "specular_transmittance": (0.2, 0.6, 0.8)},
    "tinted_uniform": {"type": "dielectric", "specular_reflectance": 0.5, "specular_transmittance": 0.25},
}


@pytest.mark.parametrize("name", sorted(DESC_CASES))
def test_xml_dielectric_flattens_to_the_mirrors_bits(hostlib, hostmirror, abi, tmp_path, name):
    """<bsdf type="dielectric"> through the XML loader and the plugin: type 3, eta = int_ior / ext_ior in fp32 (defaults 1.49 /
    1.00028, dielectric.cpp:14-16), the two spectra; bit for bit what hostmirror._bsdf_desc builds."""
    spec = DESC_CASES[name]
    tri = [((0, 0, 0), (1, 0, 0), (0, 1, 0))]
    meshes = [hostmirror.MeshSpec("glass", tri, (0.5, 0.5, 0.5), bsdf=dict(spec)), hostmirror.MeshSpec("wall", tri, (0.2, 0.3, 0.4))]
    sc = hostlib.HostScene(hostmirror.write_scene_xml(meshes, str(tmp_path), 16, 16, 1))
    d, r = sc.flatten().desc, hostmirror.flatten(meshes, 16, 16).desc
    assert d.n_bsdfs == r.n_bsdfs == 2
    b = d.bsdfs[d.meshes[0].bsdf_id]
    int_ior, ext_ior = F32(spec.get("int_ior", 1.49)), F32(spec.get("ext_ior", 1.00028))
    assert b.type == abi.MSK_BSDF_DIELECTRIC == 3 and b.back_bsdf == -1
    assert F32(b.ior_eta) == int_ior / ext_ior and F32(b.ior_inv_eta) == ext_ior / int_ior
    for i in range(2):
        assert bytes(d.bsdfs[i]) == bytes(r.bsdfs[i]), i
    if name == "tinted_uniform":
        assert (b.specular_reflectance.scale, b.specular_transmittance.scale) == (0.5, 0.25) and np.isinf(b.specular_reflectance.coeff[2])
    sc.close()


def test_twosided_dielectric_is_refused(hostlib, hostmirror, tmp_path):
    """twosided.cpp:33-35: no BSDF with a transmission component under "twosided" — in the XML loader and in the mirror"""
    tri = [((0, 0, 0), (1, 0, 0), (0, 1, 0))]
    xml = hostmirror.write_scene_xml([hostmirror.MeshSpec("glass", tri, (0.5, 0.5, 0.5), bsdf={"type": "dielectric"})], str(tmp_path), 16, 16, 1)
    text = open(xml).read()
    assert '<bsdf type="dielectric">' in text
    text = text.replace('<bsdf type="dielectric">', '<bsdf type="twosided"><bsdf type="dielectric">').replace("</bsdf>", "</bsdf></bsdf>", 1)
    (tmp_path / "two.xml").write_text(text)
    with pytest.raises(hostlib.HostError) as e:
        hostlib.HostScene(str(tmp_path / "two.xml"))
    assert "Only materials without a transmission component can be nested!" in str(e.value)
    with pytest.raises(ValueError) as e:
        hostmirror.flatten([hostmirror.MeshSpec("glass", tri, (0.5, 0.5, 0.5), bsdf={"type": "dielectric", "twosided": True})], 16, 16)
    assert "transmission" in str(e.value)


def test_reference_fresnel_self_checks(hostmirror):
    """dielectric_ref in float64 against what is known without it"""
    theta = np.radians(np.linspace(0.0, 89.9, 900))
    for eta in (1.5, 1.33, 1.49 / 1.00028, 2.4):
        # R + T = 1 with the textbook transmittance (the plugin's T is 1 - R by definition), R in [0, 1], and the same R for
        # the refracted ray arriving from inside
        assert np.allclose(D.fresnel_textbook(theta, 1.0, eta) + D.transmittance_textbook(theta, 1.0, eta), 1.0, rtol=0, atol=1e-12)
        r, ct, eta_it, eta_ti = D.fresnel(np.cos(theta), eta)
        assert np.all((r >= 0) & (r <= 1)) and np.all(ct < 0) and np.all(eta_it == eta) and np.all(eta_ti == 1 / eta)
        assert np.allclose(np.sin(theta) ** 2, eta * eta * (1 - ct * ct), rtol=0, atol=1e-14)                # Snell, squared
        r_back = D.reflectance(ct, eta)                                                                      # reciprocity of the interface
        assert np.allclose(r, r_back, rtol=1e-12, atol=1e-15)
        # the textbook unpolarised formula, from both sides
        assert np.allclose(r, D.fresnel_textbook(theta, 1.0, eta), rtol=1e-12, atol=1e-15)
        assert np.allclose(D.reflectance(-np.cos(theta), eta), D.fresnel_textbook(theta, eta, 1.0), rtol=1e-9, atol=1e-13)
        assert abs(D.reflectance(1.0, eta) - ((eta - 1) / (eta + 1)) ** 2) < 1e-15                           # normal incidence
        # total internal reflection is exactly beyond asin(1 / eta)
        tc = D.critical_angle(eta)
        assert np.all(D.reflectance(-np.cos(np.linspace(tc + 1e-9, np.pi / 2, 200)), eta) == 1.0)
        below = D.reflectance(-np.cos(np.linspace(0.0, tc - 1e-6, 200)), eta)
        assert np.all(below < 1.0) and below[-1] > 0.9
        # the slab series sums to 1
        refl, trans = D.slab_series(r[r <= 0.9], 400)                  # (0.9^800 < 1e-36: converged)
        assert (r <= 0.9).sum() > 800 and np.allclose(refl + trans, 1.0, rtol=0, atol=1e-12)
        mean, second = D.slab_roulette_moments(r[r <= 0.9])
        assert np.allclose(mean, 1.0, rtol=0, atol=1e-12) and np.all(second >= 1.0)
    assert D.reflectance(0.0, 1.5) == 1.0 and np.all(D.reflectance(np.array([0.3, -0.3, 0.0]), 1.0) == 0.0)     # fresnel.h:57-58
    # the moments of the wavelength sample: the mean is radiometry_ref's expectation, the variance is positive and converged
    flat = hostmirror.flatten([], 8, 8)
    cie = tables(flat.desc)
    spec = R.regular(360, 830, [0.5, 1.0, 2.0, 1.5])
    m1, var = D.wavelength_sample_moments(spec, cie, 16)
    m1b, varb = D.wavelength_sample_moments(spec, cie, 32)
    assert np.allclose(m1, R.expected_xyz(spec, cie, 16), rtol=1e-9) and np.allclose(var, varb, rtol=1e-6) and np.all(var > 0)
    # against the plain midpoint rule with 2^20 points, which knows nothing of the kinks
    u = (np.arange(1 << 20) + 0.5) / (1 << 20)
    g = sum(R.cmf(cie, R.wavelength_of(np.mod(u + q / 4, 1.0))) * (spec(R.wavelength_of(np.mod(u + q / 4, 1.0))) *
                                                                     R.wavelength_weight(R.wavelength_of(np.mod(u + q / 4, 1.0)))) for q in range(4)) / 4
    assert np.allclose(g.var(axis=-1), var, rtol=1e-3)


# ============================================================================= GPU
def sample(abi, gpu_ctx, flat, pixels, spp, seed, **kw):
    sc = abi.Scene(gpu_ctx, flat)
    try:
        return sc.sample_pixels(abi.render_params(spp, seed=seed, **kw), np.asarray(pixels, np.int32))
    finally:
        sc.close()


def ratios(xyz, ref):
    """Per-sample ratio to the companion, one number per sample: every channel whose companion value is positive must give it
    (asserted by the callers through `spread`); -> (ratio from Y, the largest relative disagreement between channels)"""
    xyz, ref = xyz.reshape(-1, 3).astype(np.float64), ref.reshape(-1, 3).astype(np.float64)
    assert np.all(ref >= 0) and np.all(ref[:, 1] > 0)
    assert np.all(xyz[ref == 0] == 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        q = xyz / ref
    y = q[:, 1]
    ok = (ref > 0) & (y[:, None] > 0)
    spread = np.where(ok, np.abs(q / np.where(y[:, None] > 0, y[:, None], 1.0) - 1.0), 0.0).max()
    assert np.all(xyz[(y == 0)] == 0)
    return y, spread


def classify(y, values, events):
    """Every ratio is one of `values` within EPS * (1 + events) -> the index of the value per sample"""
    values = np.asarray(values, np.float64)
    idx = np.abs(y[:, None] / values[None, :] - 1.0).argmin(-1)
    err = np.abs(y / values[idx] - 1.0)
    tol = EPS * (1 + events)
    print("DIELECTRIC ratios: values %s counts %s worst error %.3g tol %.3g" % (values.tolist(), np.bincount(idx, minlength=len(values)).tolist(), err.max(), tol))
    assert err.max() <= tol, (err.max(), tol, y[err.argmax()])
    return idx


def binomial(count, r, cap=None, what=""):
    mean, half = r.sum(), 5.0 * np.sqrt((r * (1.0 - r)).sum()) + 1.0
    print("DIELECTRIC binomial %s: N %d count %d sum R %.2f half-width %.2f (%.3g of sum R)" % (what, len(r), count, mean, half, half / max(mean, 1e-300)))
    if cap is not None:
        assert half <= cap * mean, (half, mean)
    assert abs(count - mean) <= half, (count, mean, half)


def pixels_at(desc, size, degrees, n, normal=(0.0, 1.0, 0.0), sign=1.0):
    """The n pixels of the size x size film whose centre ray meets the plane closest to `degrees` of incidence"""
    yy, xx = np.meshgrid(np.arange(size) + 0.5, np.arange(size) + 0.5, indexing="ij")
    cos = sign * D.incidence_cosines(desc, np.stack([xx, yy], -1), normal)
    order = np.argsort(np.abs(np.degrees(np.arccos(np.clip(cos, -1, 1))) - degrees), axis=None)[:n]
    return np.stack([order % size, order // size], -1).astype(np.int32)


ABOVE = dict(fov=80.0, near=0.01, far=1000.0, origin=(0, 1, 0), target=(np.sin(np.radians(42.5)), 1 - np.cos(np.radians(42.5)), 0), up=(0, 0, 1))
BELOW = dict(fov=80.0, near=0.01, far=1000.0, origin=(0, -1, 0), target=(np.sin(np.radians(42.5)), -1 + np.cos(np.radians(42.5)), 0), up=(0, 0, 1))
SIZE = 64


def interface_scenes(hm, camera, bsdf=GLASS):
    """A large quad of glass in the plane y = 0, its outside up, in the default (D65) environment; and the companion: the
    environment alone (a small diffuse quad far behind the camera keeps the scene non-empty)"""
    far = hm.MeshSpec("far", [quad((-900, 900 * np.sign(camera["origin"][1]), 0), (1, 0, 0), (0, 0, 1))], 0.5)
    glass = hm.MeshSpec("glass", [up_quad(0.0, 1000.0)], 0.5, bsdf=dict(bsdf))
    env = {"radiance": None}
    return hm.flatten([far, glass], SIZE, SIZE, camera=camera, env=env), hm.flatten([far], SIZE, SIZE, camera=camera, env=env)


def interface_case(abi, gpu_ctx, flat, ref, pixels, spp, seed, values, r_of_cos, reflected, sign=1.0, cap=None, what=""):
    xyz, pos = sample(abi, gpu_ctx, flat, pixels, spp, seed, **NO_RR)
    base, bpos = sample(abi, gpu_ctx, ref, pixels, spp, seed, **NO_RR)
    assert np.array_equal(pos, bpos)
    y, spread = ratios(xyz, base)
    assert spread <= 4 * EPS
    idx = classify(y, values, 1)
    cos = sign * D.incidence_cosines(flat.desc, pos.reshape(-1, 2).astype(np.float64))
    assert np.all(cos > 0.05)                                   # every camera ray meets the quad
    binomial(int((idx == reflected).sum()), r_of_cos(cos), cap, what)


@pytest.mark.gpu
@pytest.mark.parametrize("degrees", [10, 45, 60, 75])
def test_one_interface_from_outside(gpu_ctx, abi, hostmirror, degrees):
    """Every sample is the environment's times 1 (reflected) or times float32(1 / eta)^2 (transmitted, radiance mode); the
    reflected count is binomial with the float64 Fresnel term at each sample's own incidence.  The 60 degree group carries
    the sample count at which the 5-sigma half-width is below 1 % of the expected count (asserted first)."""
    flat, ref = interface_scenes(hostmirror, ABOVE)
    big = degrees == 60
    pixels = pixels_at(flat.desc, SIZE, degrees, 3 if big else 4)
    t = float(F32(1.0) / F32(ETA)) ** 2
    interface_case(abi, gpu_ctx, flat, ref, pixels, (1 << 20) if big else (1 << 17), 100 + degrees, [1.0, t],
                   lambda c: D.reflectance(c, ETA), 0, cap=0.01 if big else None, what="outside %d deg" % degrees)


@pytest.mark.gpu
def test_one_interface_from_inside(gpu_ctx, abi, hostmirror):
    """The camera in the dense medium.  Beyond asin(1 / eta) = 41.8 degrees every sample is reflected (ratio 1); inside,
    a sample is reflected or leaves with the weight float32(eta)^2."""
    flat, ref = interface_scenes(hostmirror, BELOW)
    cos_c = np.cos(D.critical_angle(ETA))
    # total internal reflection
    pixels = pixels_at(flat.desc, SIZE, 60, 4, sign=-1.0)
    xyz, pos = sample(abi, gpu_ctx, flat, pixels, 1 << 16, 7, **NO_RR)
    base, _ = sample(abi, gpu_ctx, ref, pixels, 1 << 16, 7, **NO_RR)
    cos = -D.incidence_cosines(flat.desc, pos.reshape(-1, 2).astype(np.float64))
    assert np.all((cos > 0.05) & (cos < cos_c - 0.05))
    y, spread = ratios(xyz, base)
    assert spread <= 4 * EPS
    assert np.all(classify(y, [1.0], 1) == 0)
    # inside the cone
    pixels = pixels_at(flat.desc, SIZE, 25, 4, sign=-1.0)
    values = [1.0, float(F32(ETA)) ** 2]
    xyz, pos = sample(abi, gpu_ctx, flat, pixels, 1 << 17, 8, **NO_RR)
    base, _ = sample(abi, gpu_ctx, ref, pixels, 1 << 17, 8, **NO_RR)
    cos = -D.incidence_cosines(flat.desc, pos.reshape(-1, 2).astype(np.float64))
    assert np.all(cos > cos_c + 0.05)
    y, spread = ratios(xyz, base)
    assert spread <= 4 * EPS
    idx = classify(y, values, 1)
    binomial(int((idx == 0).sum()), D.reflectance(-cos, ETA), what="inside 25 deg")


@pytest.mark.gpu
def test_tints(gpu_ctx, abi, hostmirror):
    """specular_reflectance 0.5 and specular_transmittance 0.25 (uniform spectra): ratios in {0.5, 0.25 / eta^2}"""
    flat, ref = interface_scenes(hostmirror, ABOVE, dict(GLASS, specular_reflectance=0.5, specular_transmittance=0.25))
    pixels = pixels_at(flat.desc, SIZE, 60, 4)
    eta_ti = float(F32(1.0) / F32(ETA))
    interface_case(abi, gpu_ctx, flat, ref, pixels, 1 << 17, 21, [0.5, 0.25 * eta_ti * eta_ti], lambda c: D.reflectance(c, ETA), 0, what="tints")


SLAB_CAMERA = dict(fov=50.0, near=0.01, far=1000.0, origin=(0, 3, 0), target=(0.3, 0, 0.2), up=(0, 0, 1))


def slab_scenes(hm, size, env):
    """Two parallel quads of glass, 100 x 100 and 1 apart, normals outward: a slab; the camera above it sees nothing else"""
    far = hm.MeshSpec("far", [quad((-900, 900, 0), (1, 0, 0), (0, 0, 1))], 0.5)
    top = hm.MeshSpec("top", [up_quad(0.5, 50.0)], 0.5, bsdf=dict(GLASS))
    bottom = hm.MeshSpec("bottom", [down_quad(-0.5, 50.0)], 0.5, bsdf=dict(GLASS))
    return hm.flatten([far, top, bottom], size, size, camera=SLAB_CAMERA, env=env), hm.flatten([far], size, size, camera=SLAB_CAMERA, env=env)


SLAB_PIXELS = [(5, 7), (31, 33), (58, 12), (20, 60)]


def slab_r(flat, pos):
    cos = D.incidence_cosines(flat.desc, pos.reshape(-1, 2).astype(np.float64))
    assert np.all(cos > 0.7)                                    # within 45 degrees: the rays meet the slab well inside its faces
    return D.reflectance(cos, ETA)


@pytest.mark.gpu
def test_lossless_slab(gpu_ctx, abi, hostmirror):
    """Whatever the path does inside the slab, it leaves with the environment's radiance: the eta^2 of entering and of leaving
    cancel, and eta stays out of the throughput.  Events of a path: R(theta) <= 0.1 within 45 degrees, so one of the 2^20
    samples has more than 15 internal reflections with probability < 1e-9; the bound counts 15 + 2 events."""
    flat, ref = slab_scenes(hostmirror, SIZE, {"radiance": None})
    xyz, pos = sample(abi, gpu_ctx, flat, SLAB_PIXELS, 1 << 18, 31, **NO_RR)
    base, _ = sample(abi, gpu_ctx, ref, SLAB_PIXELS, 1 << 18, 31, **NO_RR)
    r = slab_r(flat, pos)
    m = 15
    assert r.max() <= 0.1 and xyz.size // 3 * r.max() ** m < 1e-9
    y, spread = ratios(xyz, base)
    assert spread <= 4 * EPS
    assert np.all(classify(y, [1.0], m + 2) == 0)


@pytest.mark.gpu
def test_slab_with_russian_roulette(gpu_ctx, abi, hostmirror):
    """rr_depth 2: a path that leaves after k segments inside the slab has survived k tests at q = 0.95 (thr * eta^2 = 1 inside)
    and carries 0.95^-k; the others are 0.  The mean ratio is 1 within 5 sqrt(V / N), V from the path-length law in float64
    (dielectric_ref.slab_roulette_moments) at every sample's own incidence; the tolerance is capped at 2e-3."""
    flat, ref = slab_scenes(hostmirror, SIZE, {"radiance": None})
    kw = dict(max_depth=-1, rr_depth=2)
    xyz, pos = sample(abi, gpu_ctx, flat, SLAB_PIXELS, 1 << 18, 41, **kw)
    base, _ = sample(abi, gpu_ctx, ref, SLAB_PIXELS, 1 << 18, 41, **kw)
    y, spread = ratios(xyz, base)
    assert spread <= 4 * EPS
    q = float(F32(0.95))
    live = y > 0
    k = np.rint(np.log(y[live]) / -np.log(q))
    assert k.min() >= 0 and k.max() < 64
    err = np.abs(y[live] * q ** k - 1.0)
    tol = EPS * (1 + np.where(k == 0, 1, k + 1))               # k = 0: one reflection; else entering, k - 1 reflections, leaving
    print("DIELECTRIC roulette: k histogram %s dead %d worst error/tol %.3g" % (np.bincount(k.astype(int)).tolist(), int((~live).sum()), (err / tol).max()))
    assert np.all(err <= tol)
    mean, second = D.slab_roulette_moments(slab_r(flat, pos), q)
    n = len(y)
    tol_mean = 5.0 * np.sqrt((second - mean * mean).mean() / n) + EPS * 3
    print("DIELECTRIC roulette: N %d mean ratio %.6f tol %.3g" % (n, y.mean(), tol_mean))
    assert tol_mean <= 2e-3
    assert abs(y.mean() - 1.0) <= tol_mean


@pytest.mark.gpu
def test_delta_mis_of_an_area_emitter(gpu_ctx, abi, hostmirror):
    """No environment; the mirror direction of every pixel meets the front of a large area emitter the camera does not see.
    A reflected sample carries the emitter's radiance with MIS weight 1 (path.cpp:104-106: the emitter pdf of a delta lobe is
    0) = the companion's value (the emitter filling the view, max_depth 1); a transmitted one carries nothing.  A value in
    between is the rule missing."""
    hm = hostmirror
    cam = dict(fov=20.0, near=0.01, far=1000.0, origin=(-2, 2, 0), target=(0, 0, 0), up=(0, 0, 1))
    rad = (0.9, 0.5, 0.2)
    glass = hm.MeshSpec("glass", [up_quad(0.0, 1000.0)], 0.5, bsdf=dict(GLASS))
    light = hm.MeshSpec("light", [quad((50, 100.5, 0), (0, 0, 100), (0, 100, 0))], 0.0, radiance=rad)      # z x y = -x: faces the glass
    flat = hm.flatten([glass, light], 32, 32, camera=cam)
    wall = hm.MeshSpec("light", [quad((0, -5, 0), (0, 0, 100), (100, 0, 0))], 0.0, radiance=rad)            # faces up, fills the view
    ref = hm.flatten([wall], 32, 32, camera=cam)
    pixels = [(2, 3), (16, 16), (29, 8), (10, 28)]
    xyz, pos = sample(abi, gpu_ctx, flat, pixels, 1 << 17, 51, **NO_RR)
    base, _ = sample(abi, gpu_ctx, ref, pixels, 1 << 17, 51, max_depth=1)
    # the geometry in float64: every camera ray meets the glass, every mirrored ray the emitter's face
    o, d = R.camera_ray(flat.desc, pos.reshape(-1, 2)[:, 0].astype(np.float64), pos.reshape(-1, 2)[:, 1].astype(np.float64))
    assert np.all(d[:, 1] < 0)
    x = R.hit_plane(o, d, (0, 0, 0), (0, 1, 0))
    m = d * np.array([1.0, -1.0, 1.0])
    t = (50.0 - x[:, 0]) / m[:, 0]
    hit = x + m * t[:, None]
    assert np.all(m[:, 0] > 0) and np.all((hit[:, 1] > 1.0) & (hit[:, 1] < 200.0) & (np.abs(hit[:, 2]) < 99.0))
    xyz, base = xyz.reshape(-1, 3).astype(np.float64), base.reshape(-1, 3).astype(np.float64)
    assert np.all(base[:, 1] > 0)
    lit = xyz[:, 1] != 0
    assert np.all(xyz[~lit] == 0)
    err = np.abs(xyz[lit] - base[lit]) / np.maximum(base[lit], 1e-300)
    err = np.where(base[lit] > 0, err, np.where(xyz[lit] == 0, 0.0, np.inf))
    print("DIELECTRIC delta MIS: N %d lit %d worst error %.3g tol %.3g" % (len(lit), int(lit.sum()), err.max(), 2 * EPS))
    assert err.max() <= 2 * EPS
    binomial(int(lit.sum()), D.reflectance(-d[:, 1], ETA), what="delta MIS")


# ----------------------------------------------------------------------------- variants
ROOM_CAMERA = dict(fov=70.0, near=0.01, far=100.0, origin=(0.1, 0.1, -0.9), target=(0.0, -0.2, 0.5), up=(0, 1, 0))
VARIANT_KEYS = ("MSK_STREAMS", "MSK_SORT", "MSK_FUSED", "MSK_LDS_SCENE_KB", "MSK_FUSED_HBM", "MSK_BVH_BUILD", "MSK_FUSED_TAIL_PCT", "MSK_WIDE_BVH", "MSK_QUANT_BVH")


def room_meshes(hm, glass):
    """A closed diffuse room (checkerboard floor), an area light under the ceiling, a rough-conductor plate, and `glass`
    (a list of meshes, last in the scene so that every other triangle keeps its index without it).  An anchor quad outside
    the room fixes the scene's extent, so that glass parked outside the room, inside that extent, changes no padding."""
    lo, hi = np.array([-1.0, -1.0, -1.0]), np.array([1.0, 1.0, 1.0])
    c, h = (lo + hi) / 2, (hi - lo) / 2
    ex, ey, ez = np.diag(h)
    walls = [("floor", c - ey, ez, ex), ("ceiling", c + ey, ex, ez), ("left", c - ex, ey, ez), ("right", c + ex, ez, ey),
             ("front", c - ez, ex, ey), ("back", c + ez, ey, ex)]
    colors = {"left": (0.57, 0.04, 0.04), "right": (0.1, 0.38, 0.08)}
    meshes = []
    for n, p, u, v in walls:
        bsdf = {"type": "diffuse", "texture": {"type": "checkerboard", "color0": (0.8, 0.8, 0.8), "color1": (0.2, 0.2, 0.3), "scale": (6, 6)}} if n == "floor" else None
        meshes.append(hm.MeshSpec(n, [quad(p, u, v)], colors.get(n, (0.7, 0.7, 0.7)), bsdf=bsdf))
    meshes.append(hm.MeshSpec("light", [quad((0, 0.98, 0), (0.3, 0, 0), (0, 0, 0.3))], 0.0, radiance=(20, 18, 15)))      # x x z = -y
    meshes.append(hm.MeshSpec("plate", [quad((-0.5, -0.6, 0.4), (0, 0, 0.3), (0.3, 0.1, 0))], 0.5,
                              bsdf={"type": "roughconductor", "alpha": 0.2, "eta": (0.2, 0.92, 1.1), "k": (3.9, 2.45, 2.14)}))
    meshes.append(hm.MeshSpec("anchor", [quad((9.5, 0, 0), (0, 0.5, 0), (0, 0, 0.5))], 0.5))
    return meshes + list(glass)


def glass_box(hm, c):
    return [hm.MeshSpec("glassbox", box(c, (0.25, 0.3, 0.2)), 0.5, bsdf={"type": "dielectric"})]


def render_under(abi, gpu_ctx, monkeypatch, flat, env, prm):
    for k in VARIANT_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)                                # (MSK_LDS_SCENE_KB / MSK_BVH_BUILD: read by msk_gpu_scene_create)
    sc = abi.Scene(gpu_ctx, flat)
    try:
        film, st = sc.render(prm)
    finally:
        sc.close()
        for k in env:
            monkeypatch.delenv(k, raising=False)
    return film, st


LDS_VARIANTS = [{}, {"MSK_STREAMS": "1"}, {"MSK_SORT": "0"}, {"MSK_FUSED": "1"}, {"MSK_LDS_SCENE_KB": "0"},
                {"MSK_LDS_SCENE_KB": "0", "MSK_FUSED_HBM": "1"}, {"MSK_BVH_BUILD": "gpu"}]


@pytest.mark.gpu
def test_variants_agree_bit_for_bit(gpu_ctx, abi, hostmirror, monkeypatch):
    """A mixed, LDS-resident scene under every execution variant: one film.  And the scene with its glass box parked where no
    ray goes (outside the closed room) renders the film of the scene without the box, which runs the kernels without the
    dielectric code."""
    hm = hostmirror
    prm = abi.render_params(spp=16, seed=3)
    flat = hm.flatten(room_meshes(hm, glass_box(hm, (0.35, -0.69, 0.2))), 64, 64, camera=ROOM_CAMERA)
    films = []
    for env in LDS_VARIANTS:
        film, st = render_under(abi, gpu_ctx, monkeypatch, flat, env, prm)
        assert st.samples == 64 * 64 * 16 and st.invalid_samples == 0 and np.isfinite(film).all(), env
        films.append(film)
    assert films[0][..., :3].max() > 0
    for env, film in zip(LDS_VARIANTS[1:], films[1:]):
        assert np.array_equal(film.view(np.uint32), films[0].view(np.uint32)), env
    parked, _ = render_under(abi, gpu_ctx, monkeypatch, hm.flatten(room_meshes(hm, glass_box(hm, (5.0, 0.0, 0.0))), 64, 64, camera=ROOM_CAMERA), {}, prm)
    without, _ = render_under(abi, gpu_ctx, monkeypatch, hm.flatten(room_meshes(hm, []), 64, 64, camera=ROOM_CAMERA), {}, prm)
    assert np.array_equal(parked.view(np.uint32), without.view(np.uint32))
    assert not np.array_equal(films[0].view(np.uint32), without.view(np.uint32))       # the box in the room is seen


@pytest.mark.gpu
def test_variants_agree_with_the_tables_in_hbm(gpu_ctx, abi, hostmirror, monkeypatch):
    """The same with a glass blob of ~770 triangles: tree and per-triangle tables stay in HBM, so k_shade_gen_d<false> and, for
    the thin end or (MSK_FUSED=1) the whole pass, k_wavefront_h_d run."""
    hm = hostmirror
    prm = abi.render_params(spp=16, seed=4)
    blob = hm.blob_mesh("blob", (0.3, -0.5, 0.2), 0.35, 16, 24, 0.5)
    blob.bsdf = {"type": "dielectric", "int_ior": 1.33}
    flat = hm.flatten(room_meshes(hm, [blob]), 64, 64, camera=ROOM_CAMERA)
    assert flat.desc.n_faces * 96 > 40 * 1024
    films = []
    variants = [{}, {"MSK_FUSED_HBM": "0"}, {"MSK_FUSED": "1"}, {"MSK_SORT": "0", "MSK_STREAMS": "1"}, {"MSK_FUSED_TAIL_PCT": "50"}, {"MSK_BVH_BUILD": "gpu"}]
    for env in variants:
        film, st = render_under(abi, gpu_ctx, monkeypatch, flat, env, prm)
        assert st.samples == 64 * 64 * 16 and st.invalid_samples == 0 and np.isfinite(film).all(), env
        films.append(film)
    assert films[0][..., :3].max() > 0
    for env, film in zip(variants[1:], films[1:]):
        assert np.array_equal(film.view(np.uint32), films[0].view(np.uint32)), env


# ----------------------------------------------------------------------------- MSK_RNG_PCG_BLOCK
@pytest.mark.gpu
def test_pcg_block_slab_film_matches_the_closed_form(gpu_ctx, abi, hostmirror):
    """The slab through k_path_serial_d (the scalar loop's draw order: no next2d() at a dielectric hit): sum(XYZ) / sum(W) of
    rendered films against the environment's own XYZ.  With Russian roulette off every path carries the environment's radiance,
    so a sample's only spread is that of its wavelength sample, whose variance is a float64 quadrature
    (dielectric_ref.wavelength_sample_moments).  Films of consecutive seeds are summed in float64 until 5 sigma / sqrt(N) + the
    quadrature's error + the fp32 terms fit under 2e-3 |E| in Y and 4e-3 in X and Z (asserted first).

    N counts INDEPENDENT samples.  Every image block of a render seeds its PCG32 stream alike (independent.cpp as the oracle
    pins it: one seed per render), and the slab's paths are nearly all of one length, so the blocks of a film walk the same
    stream almost in step: a first version of this test that took the 256 blocks of a 128 x 128 film at block_size 8 for
    independent missed X by 6.1 of its sigmas (dev / |E| 6.4e-4 against 5 sigma = 4.0e-4).  So a film is ONE block here
    (block_size = the film's size: one stream, every draw used once), at the price of one working lane: Z needs 4e5 samples
    (sigma / mean 0.46: one of the four wavelengths of a sample meets the blue lobe) at 13 us each, five seconds in all.
    N = the samples whose whole filter footprint lies on the film (the others add a smaller weight, which never lowers
    (sum w)^2 / sum w^2: the argument of S5 in test_radiometry_closed_form); fp32: 2e-5 inside a sample (a handful of
    bounces), spp * 25 * 2^-24 in a film pixel's sum."""
    hm = hostmirror
    table = (360, 830, [0.5, 1.0, 2.0, 1.5])
    size, spp, border = 64, 16, 2
    flat, _ = slab_scenes(hm, size, {"radiance": hm.Regular(*table)})
    cie = tables(flat.desc)
    spec = R.regular(*table)
    e, var = D.wavelength_sample_moments(spec, cie, 16)
    e2, var2 = D.wavelength_sample_moments(spec, cie, 32)
    quad_err = np.abs(e - e2)
    assert np.all(quad_err <= 1e-6 * np.abs(e2)) and np.allclose(var, var2, rtol=1e-4) and np.allclose(e2, R.expected_xyz(spec, cie, 32), rtol=1e-9)
    caps = np.array([4e-3, 2e-3, 4e-3])
    fp32 = 2e-5 + spp * (2 * border + 1) ** 2 * 2.0 ** -24
    per_film = spp * (size - 2 * border) ** 2
    room_ = (caps - fp32) * np.abs(e2) - quad_err
    n_films = int(np.ceil(((5.0 * np.sqrt(var2) / (0.95 * room_)) ** 2).max() / per_film))
    assert 1 <= n_films <= 8, n_films
    n = n_films * per_film
    tol = 5.0 * np.sqrt(var2 / n) + quad_err + fp32 * np.abs(e2)
    assert np.all(tol <= caps * np.abs(e2)), (tol / np.abs(e2)).tolist()
    total = np.zeros(5)
    sc = abi.Scene(gpu_ctx, flat)
    try:
        for k in range(n_films):
            film, st = sc.render(abi.render_params(spp, seed=900 + k, rng_mode=abi.MSK_RNG_PCG_BLOCK, block_size=size, **NO_RR))
            assert film.shape == (size, size, 5) and st.samples == size * size * spp and st.invalid_samples == 0
            assert st.shadow_rays == 0                          # no next-event sample anywhere: every surface a ray can meet is glass
            total += film.astype(np.float64).sum((0, 1))
    finally:
        sc.close()
    mean = total[:3] / total[4]
    print("DIELECTRIC pcg slab: films %d N %d expected %s estimate %s dev/|E| %s tol/|E| %s" % (
        n_films, n, e2.tolist(), mean.tolist(), (np.abs(mean - e2) / np.abs(e2)).tolist(), (tol / np.abs(e2)).tolist()))
    assert np.all(np.abs(mean - e2) <= tol)


# ----------------------------------------------------------------------------- msk_gpu_scene_create
@pytest.mark.gpu
def test_scene_create_refusals(gpu_ctx, abi, hostmirror):
    hm = hostmirror
    tri = [((0, 0, 0), (1, 0, 0), (0, 1, 0))]

    def flat_with(edit):
        flat = hm.flatten([hm.MeshSpec("glass", tri, 0.5, bsdf={"type": "dielectric"})], 16, 16)
        edit(flat.desc.bsdfs[0])
        return flat

    def set_back(b): b.back_bsdf = 0
    def set_eta(b): b.ior_eta = 0.0
    def set_inv(b): b.ior_inv_eta = -1.0
    def set_type(b): b.type = 4
    for edit, needle in ((set_back, "Only materials without a transmission component can be nested!"),
                         (set_eta, "the relative index of refraction must be positive"),
                         (set_inv, "the relative index of refraction must be positive"),
                         (set_type, "type 4 is not supported")):
        with pytest.raises(abi.MskError) as e:
            abi.Scene(gpu_ctx, flat_with(edit)).close()
        assert needle in str(e.value), str(e.value)
    abi.Scene(gpu_ctx, flat_with(lambda b: None)).close()       # and unedited it is accepted
