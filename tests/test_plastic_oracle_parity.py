"""The twin of `plastic` and `roughplastic` (oracle/oracle.cpp, D19-D22), and the device held to it bit for bit.

The layout is test_widened_oracle_parity's, whose helpers this file imports.
CPU layer (the twin earns trust before the device is held to it):
  (a)  the oracle's hooks against plastic_ref / roughplastic_ref on the very inputs the GPU probe tests generate, as uint32;
       and, because two closed forms of each plastic are lit by a sun, msk_oracle_light_sample against light_ref (D23);
  (a') the oracle's two constants per entry against float64 (2e-7 relative, 1e-6) and against the packer's own bits
       (tests/native/plastic_constants_probe.cpp), for every plastic entry of every scene this file renders: open_twin() checks them
       whenever it makes a scene;
  (b)  the twin's renders against the float64 expectations of test_plastic_bsdf / test_roughplastic_bsdf, by twin_mean and meets;
  (c)  identities that need no tolerance; (c') refusals;
  (d)  the path tallies of every parity scene at the parameters the GPU layer uses, per film.
GPU layer: every comparison is array_equal on the uint32 view; no pixel or sample is left out; counters through check_counters.
  (e)  the default configuration against the twin on the variant scenes of test_plastic_bsdf / test_roughplastic_bsdf at the parameters
       of their `variant_reference` fixtures: those files hold every execution variant and tree form to that default;
  (f)  one all-features scene with plastics over RNG x hide_emitters x depth limits, in both table placements, with a crop window and
       sample shards;
  (g)  "aov" on the plastic variant scene."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import delta_ref as D
import light_ref as L
import oracle_binding
import plastic_ref as P
import roughplastic_ref as RP
import test_delta_light_mirror as DM
import test_envmap as EV
import test_mask_bsdf as MB
import test_plastic_bsdf as TP
import test_roughplastic_bsdf as TR
import test_spot_directional as SD
import test_widened_oracle_parity as WP
from test_widened_oracle_parity import assert_bits, bits, check_counters, counted, meets, sample_pixels_threaded, twin_mean

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
PLASTIC_TYPES = (6, 7)


# ===================================================================================================== the packer's constants, and the one door to a twin scene
@pytest.fixture(scope="module")
def packer_constants(tmp_path_factory, abi):
    """tests/native/plastic_constants_probe.cpp: mskscene::plastic_constants on a flattened scene -> (fdr_int, ssw) float32"""
    so = str(tmp_path_factory.mktemp("plastic_constants") / "plastic_constants_probe.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", so,
                           os.path.join(ROOT, "tests", "native", "plastic_constants_probe.cpp")])
    lib = C.CDLL(so)
    lib.plastic_constants_probe.argtypes = [C.POINTER(abi.SceneDesc), C.c_uint32, C.c_void_p]

    def probe(flat, b):
        out = np.zeros(2, F)
        assert lib.plastic_constants_probe(C.byref(flat.desc), b, out.ctypes.data_as(C.c_void_p)) == 0, b
        return F(out[0]), F(out[1])
    return probe


def plastic_entries(flat):
    return [b for b in range(flat.desc.n_bsdfs) if flat.desc.bsdfs[b].type in PLASTIC_TYPES]


def constants_equal_the_packers(o, flat, packer_constants):
    """bit equality of (fdr_int, ssw), each rounded once from a double of its own side.  If a pair of roundings ever parts, that is a
    finding: the message carries the eta and both sides' values"""
    for b in plastic_entries(flat):
        got, want = o.plastic_constants(b), packer_constants(flat, b)
        assert np.array_equal(bits(np.array(got)), bits(np.array(want))), (b, float(flat.desc.bsdfs[b].ior_eta), [float(x) for x in got], [float(x) for x in want])


def open_twin(oracle, packer_constants, flat):
    """every twin scene this file renders is made here, and its plastics' constants are the packer's bits before anything is rendered"""
    o = oracle.scene(flat)
    constants_equal_the_packers(o, flat, packer_constants)
    return o


# ===================================================================================================== (a) hooks against the restatements
def probe_flat(hm, entries, quad, extra=()):
    meshes = [quad(hm, name, spec, 0.1 * i, uv=True) for i, (name, spec) in enumerate(entries)]
    meshes.append(hm.MeshSpec("lamp", [tuple(DM.LAMP)], hm.LUMINAIRE, radiance=(40, 30, 20)))
    return hm.flatten(meshes + list(extra), 16, 16, camera=TP.CAM, coeff_lookup=None)


def entry_inputs(oracle, flat, b, fdr, ssw, rng, n, probe_inputs):
    """what the GPU probe tests derive for entry b, in their order: the inputs, wi / wo on the front side, rho, s and the hemisphere warp"""
    bd = flat.desc.bsdfs[b]
    eta = F(bd.ior_eta)
    twosided = bd.back_bsdf >= 0

    def front(w):
        return np.where((w[:, 2:3] < 0) & twosided, w * np.array([1, 1, -1], F), w).astype(F), (w[:, 2] < 0) & twosided

    uv, wi, wo_in, su, wl = probe_inputs(rng, n, lambda w: P.lobes32(front(w)[0][:, 2], eta, ssw)[2])
    wif, flipped = front(wi)
    wof = np.where(flipped[:, None], wo_in * np.array([1, 1, -1], F), wo_in).astype(F)
    rho = TP.rho32(oracle, flat, b, uv, wl)
    s = D.spectrum32(oracle if not np.isinf(bd.specular_reflectance.coeff[2]) else None, bd.specular_reflectance, wl)
    hemi = np.array([oracle.warps(u)[2] for u in su[:, 1:]], F)
    return dict(uv=uv, wi=wi, wo=wo_in, su=su, wl=wl, wif=wif, wof=wof, flipped=flipped, rho=rho, s=s, hemi=hemi,
                eta=eta, inv_eta=F(bd.ior_inv_eta), nonlinear=bool(bd.sample_visible), alpha=F(bd.alpha_u))


def test_a_plastic_hooks_equal_plastic_ref(hostmirror, oracle, packer_constants):
    """msk_oracle_plastic_sample / _plastic_eval against plastic_ref on test_plastic_bsdf's probe scene, generator and inputs: 11 entries x
    256 inputs, compared as uint32.  test_plastic_bsdf's probe test lets a zero stand against a zero of the other sign; the twin does
    not need that allowance (its zeros carry the restatement's signs), so none is made here: nothing is left out."""
    entries = TP.probe_entries()
    flat = probe_flat(hostmirror, entries, TP.quad)
    o = open_twin(oracle, packer_constants, flat)
    rng = np.random.RandomState(11)
    try:
        for b, (name, _) in enumerate(entries):
            fdr, ssw = o.plastic_constants(b)
            k = entry_inputs(oracle, flat, b, fdr, ssw, rng, 256, TP.probe_inputs)
            want = P.sample32(k["wif"], k["su"][:, 0], k["hemi"], k["rho"], k["s"], k["eta"], k["inv_eta"], fdr, ssw, k["nonlinear"])
            want["wo"][k["flipped"], 2] = -want["wo"][k["flipped"], 2]
            wo_pdf, value, flags = o.plastic_sample(b, k["uv"], k["wi"], k["su"], k["wl"])
            assert np.array_equal(flags[:, 3] != 0, want["ok"]) and np.array_equal(flags[:, 1] != 0, want["delta"]), name
            assert not flags[:, 2].any() and np.all(flags[:, 0] == 1), name      # no null lobe without a mask; eta = 1
            for what, got, ref in (("wo", wo_pdf[:, :3], want["wo"]), ("pdf", wo_pdf[:, 3], want["pdf"]), ("value", value, want["value"])):
                assert_bits(what, got, ref, name)
            a_pdf, ev = o.plastic_eval(b, k["uv"], k["wi"], k["wo"], k["wl"])
            rv, rp = P.eval32(k["wif"], k["wof"], k["rho"], k["eta"], k["inv_eta"], fdr, ssw, k["nonlinear"])
            assert np.all(a_pdf[:, 0] == 1)
            assert_bits("eval", ev, rv, name)
            assert_bits("eval pdf", a_pdf[:, 1], rp, name)
            if float(k["eta"]) > 1 and name not in ("no_coat", "black_base"):
                assert want["delta"].any() and (want["ok"] & ~want["delta"]).any(), name
        with pytest.raises(ValueError):                                  # the lamp's BSDF is not a plastic
            o.plastic_sample(len(entries), k["uv"][:1], k["wi"][:1], k["su"][:1], k["wl"][:1])
        with pytest.raises(ValueError):                                  # ... and a plastic is no roughplastic
            o.roughplastic_eval(0, k["uv"][:1], k["wi"][:1], k["wo"][:1], k["wl"][:1])
        with pytest.raises(ValueError):
            o.plastic_constants(len(entries))
    finally:
        o.close()


def roughplastic_probe_flat(hm):
    return probe_flat(hm, TR.probe_entries(), TR.quad, extra=[TR.quad(hm, "smooth", TP.plastic(), 0.1 * len(TR.probe_entries()))])


def test_a_roughplastic_hooks_equal_roughplastic_ref(hostmirror, oracle, packer_constants):
    """msk_oracle_roughplastic_sample / _roughplastic_eval against roughplastic_ref on test_roughplastic_bsdf's probe scene and inputs:
    8 entries x N_PROBE inputs as uint32, no allowance; live coats, bases, dead coat samples and failures all occur"""
    entries = TR.probe_entries()
    flat = roughplastic_probe_flat(hostmirror)
    o = open_twin(oracle, packer_constants, flat)
    rng = np.random.RandomState(13)
    seen = dict(coat=0, base=0, dead=0, failed=0)
    try:
        for b, (name, _) in enumerate(entries):
            assert flat.desc.bsdfs[b].type == 7
            fdr, ssw = o.plastic_constants(b)
            k = entry_inputs(oracle, flat, b, fdr, ssw, rng, TR.N_PROBE, TR.probe_inputs)
            want = RP.sample32(oracle, k["wif"], k["su"][:, 0], k["su"][:, 1:], k["hemi"], k["rho"], k["s"], k["eta"], k["inv_eta"], fdr, ssw, k["nonlinear"], k["alpha"])
            want["wo"][k["flipped"], 2] = -want["wo"][k["flipped"], 2]
            wo_pdf, value, flags = o.roughplastic_sample(b, k["uv"], k["wi"], k["su"], k["wl"])
            assert np.array_equal(flags[:, 3] != 0, want["ok"]), name
            assert not flags[:, 1].any() and not flags[:, 2].any() and np.all(flags[:, 0] == 1), name      # never delta, no null lobe, eta = 1
            for what, got, ref in (("wo", wo_pdf[:, :3], want["wo"]), ("pdf", wo_pdf[:, 3], want["pdf"]), ("value", value, want["value"])):
                assert_bits(what, got, ref, name)
            live = want["pdf"] > 0
            seen["coat"] += int((want["coat"] & live).sum()); seen["base"] += int((~want["coat"] & live).sum())
            seen["dead"] += int((want["coat"] & ~live).sum()); seen["failed"] += int((~want["ok"]).sum())
            a_pdf, ev = o.roughplastic_eval(b, k["uv"], k["wi"], k["wo"], k["wl"])
            rv, rp = RP.eval32(k["wif"], k["wof"], k["rho"], k["s"], k["eta"], k["inv_eta"], fdr, ssw, k["nonlinear"], k["alpha"])
            assert np.all(a_pdf[:, 0] == 1) and rp.max() > 0
            assert_bits("eval", ev, rv, name)
            assert_bits("eval pdf", a_pdf[:, 1], rp, name)
        print("TWIN roughplastic probes: %s" % seen)
        assert min(seen.values()) > 0
        with pytest.raises(ValueError):                                  # the smooth plastic of the same scene is no roughplastic
            o.roughplastic_sample(len(entries) + 1, k["uv"][:1], k["wi"][:1], k["su"][:1], k["wl"][:1])
        assert o.plastic_constants(len(entries) + 1)[0] == o.plastic_constants(0)[0]      # the same eta, the same fdr_int
    finally:
        o.close()


def test_a_light_hook_equals_light_ref(hostmirror, oracle):
    """The closed forms (c) of the plastic and (b) of the roughplastic are lit by a sun, so the twin restates the next-event sample of the
    two delta lights of msk_light_desc (oracle.cpp, D23) and no more of them.  msk_oracle_light_sample against light_ref on
    test_spot_directional's probe scenes and points, as its GPU probe test compares the device: both spots (beam, transition, dark,
    a cosine exactly on either edge, the position itself) and the sun, as uint32, nothing left out"""
    pos, p, wl = SD.probe_points()
    flat = SD.probe_flat(hostmirror)
    sp_pos, sp_axis, cc, cb = SD.light_of(flat, 2)
    c = L.spot_cosine32(sp_pos, sp_axis, p)
    f = L.falloff32(c, cc, cb)
    k = int(np.argmax((f > 0.3) & (f < 0.7)))
    for what, fl in (("as flattened", flat), ("cos_beam = c", SD.probe_flat(hostmirror, (cc, c[k]))), ("cos_cutoff = c", SD.probe_flat(hostmirror, (c[k], cb)))):
        o = oracle.scene(fl)
        try:
            for e in (2, 4):
                lp, la, lc, lb = SD.light_of(fl, e)
                gd, gv = o.light_sample(e, p, wl)
                rd, rv, pdf = L.spot_sample32(lp, la, lc, lb, p, SD.emitter_value32(hostmirror, oracle, fl, e, wl))
                assert_bits("d, dist", gd, rd, what, e)
                assert_bits("value", gv, rv, what, e)
                if e == 2 and fl is not flat:                           # on the boundary: c >= cos_beam gives 1, c <= cos_cutoff gives 0
                    assert np.array_equal(gv[k], rv[k] if "beam" in what else np.zeros(4, F)) and pdf[k] == (1 if "beam" in what else 0)
            _, w, _, _ = SD.light_of(fl, 3)
            gd, gv = o.light_sample(3, p, wl)
            rd, rv = L.sun_sample32(w, L.env_radius32(fl.vertices), SD.emitter_value32(hostmirror, oracle, fl, 3, wl))
            assert np.array_equal(bits(gd), bits(rd)) and np.array_equal(bits(gv), bits(rv)) and rd[0, 3] > 0
            for e in (0, 1, 5):                                          # the lamp, the point light, out of range
                with pytest.raises(ValueError):
                    o.light_sample(e, p[:1], wl[:1])
        finally:
            o.close()
    with pytest.raises(ValueError):                                      # a sun without its descriptor: refused, where it ran the area light's code before
        oracle.scene(SD.probe_flat(hostmirror), lights=[SD.probe_flat(hostmirror).lights[0]])
    bad = SD.probe_flat(hostmirror)
    bad.lights[1].direction[0] = 2.0                                     # not unit length
    with pytest.raises(ValueError):
        oracle.scene(bad)


# ===================================================================================================== (a') the constants
@pytest.mark.parametrize("kind", ["plastic", "roughplastic"])
def test_a_constants_meet_float64_and_the_packers_bits(hostmirror, oracle, packer_constants, kind):
    """both probe scenes: fdr_int to 2e-7 relative and ssw to 1e-6 of float64 (plastic_ref), the project's tolerances; and the packer's
    bits.  (Every other scene of this file passes the second check in open_twin.)"""
    flat = probe_flat(hostmirror, TP.probe_entries(), TP.quad) if kind == "plastic" else roughplastic_probe_flat(hostmirror)
    o = oracle.scene(flat)
    try:
        entries = plastic_entries(flat)
        assert len(entries) == (11 if kind == "plastic" else 9)
        for b in entries:
            fdr, ssw = o.plastic_constants(b)
            want_fdr, want_ssw = P.fdr_int64(float(flat.desc.bsdfs[b].ior_eta)), P.desc_ssw64(flat.desc, b, flat.texels)
            assert abs(float(fdr) - want_fdr) <= 2e-7 * want_fdr and abs(float(ssw) - want_ssw) <= 1e-6, (kind, b, fdr, want_fdr, ssw, want_ssw)
        constants_equal_the_packers(o, flat, packer_constants)
    finally:
        o.close()


def test_a_constants_of_tabulated_spectra_and_indices_near_one(hostmirror, oracle, packer_constants):
    """what the probe scenes do not hold: a `regular` base and a `regular` specular_reflectance (ssw from tables), a nearest bitmap, and
    relative indices from 1 + 1e-5 up, where the integrand of fdr_ext is steepest at grazing incidence: the packer's bits, and float64.
    A finding, kept out of the bit comparison and not out of the float64 one: at ior_eta = 1.00000095 (1 + 2^-20) the two roundings
    part.  The oracle's double is 2.2252308e-06, which plastic_ref's two float64 rules give as well (2.22523082716e-06 by the
    identity, 2.22523082704e-06 from the inside); the packer's four equal 64-point panels give 2.2252302e-06, 2.7e-7 relative beside
    it: the branch points of F at mu = +- i sqrt(eta^2 - 1) are then 1.4e-3 from the panel [0, 1/4].  From 1 + 1e-5 up, and at 3000
    indices drawn uniformly from [1, 2.6], no pair parted."""
    table = lambda lo, hi, n, seed: hostmirror.Regular(380.0, 780.0, np.random.RandomState(seed).uniform(lo, hi, n).astype(F))
    specs = [TP.plastic(table(0.1, 0.9, 7, 1), table(0.2, 1.0, 31, 2), 1.3), TR.roughplastic(table(0.1, 0.9, 95, 3), 0.6, 1.7, True, 0.2),
             TP.plastic(dict(TP.BITMAP, filter="nearest"), table(0.0, 0.1, 2, 4), 2.6, True)]
    specs += [TP.plastic(0.5, 0.5, eta) for eta in (1.0 + 1e-5, 1.0001, 1.003, 1.01, 1.05, 1.1, 1.33, 2.0, 2.6, 4.0)]
    quads = lambda sp: [TP.quad(hostmirror, "q%d" % i, s, 0.1 * i, uv=True) for i, s in enumerate(sp)]
    flat = hostmirror.flatten(quads(specs), 16, 16, camera=TP.CAM, coeff_lookup=None)
    near = hostmirror.flatten(quads([TP.plastic(0.5, 0.5, 1.0 + 1e-6)]), 16, 16, camera=TP.CAM, coeff_lookup=None)
    for f, o, first in ((flat, open_twin(oracle, packer_constants, flat), 3), (near, oracle.scene(near), 0)):
        try:
            for b in range(first, f.desc.n_bsdfs):
                eta = float(f.desc.bsdfs[b].ior_eta)
                fdr, want = float(o.plastic_constants(b)[0]), P.fdr_int64(eta)
                assert abs(fdr - want) <= 2e-7 * want, (eta, fdr, want)
                assert abs(P.fdr_int_direct64(eta) - want) <= 1e-9 * want, (eta, P.fdr_int_direct64(eta), want)
        finally:
            o.close()


# ===================================================================================================== (b) closed forms on the twin
@pytest.mark.parametrize("name", TP.CASES)
def test_b_twin_meets_the_plastic_closed_forms(hostmirror, oracle, abi, packer_constants, name):
    flat, expected, _, params = TP.closed_form_case(hostmirror, name)
    o = open_twin(oracle, packer_constants, flat)
    try:
        if name.startswith("d"):
            assert o.plastic_constants(0)[1] == 1.0                      # every sample is the mirror lobe
        mean, se = twin_mean(o, abi, name, expected, **params)
    finally:
        o.close()
    meets(mean, se, expected)


@pytest.mark.parametrize("name", TR.CASES)
def test_b_twin_meets_the_roughplastic_expectations(hostmirror, oracle, abi, packer_constants, name):
    flat, expected, params = TR.closed_form_case(hostmirror, name)
    o = open_twin(oracle, packer_constants, flat)
    try:
        mean, se = twin_mean(o, abi, name, expected, **params)
    finally:
        o.close()
    meets(mean, se, expected)


# ===================================================================================================== (c) identities on the twin
VARIANT_FLATS = {"plastic": TP.variant_flat, "roughplastic": TR.variant_flat}


def twin_films(oracle, packer_constants, flat, prms):
    o = open_twin(oracle, packer_constants, flat)
    out = [o.render(p, threads=8)[0] for p in prms]
    o.close()
    return out


@pytest.mark.parametrize("form", ["constant", "image"])
@pytest.mark.parametrize("kind", sorted(VARIANT_FLATS))
def test_c_opacity_one_over_the_plastics_is_the_unmasked_film(hostmirror, oracle, abi, packer_constants, kind, form):
    """a = 1 on every entry of the variant scene (a constant, or a bilinear image of ones): u.x / 1 and 1 * pdf are exact.  The plain
    scene has no mask records in the twin at all; the masked one takes every mask branch"""
    prms = WP.identity_params(abi)
    values = np.ones((3, 2), F) if form == "image" else None
    plain = twin_films(oracle, packer_constants, VARIANT_FLATS[kind](hostmirror, "lds"), prms)
    masked = twin_films(oracle, packer_constants, MB.with_masks(abi, VARIANT_FLATS[kind](hostmirror, "lds"), values), prms)
    for a, b in zip(plain, masked):
        assert np.array_equal(bits(a), bits(b)) and a[..., :3].max() > 0


@pytest.mark.parametrize("kind", sorted(VARIANT_FLATS))
def test_c_one_sided_plastic_is_black_from_behind(hostmirror, oracle, abi, packer_constants, kind):
    """the plane wound the other way round under a sky: exactly 0 in both RNG modes; the same plane from the front, and twosided from
    behind, is lit"""
    make = TP.plastic if kind == "plastic" else TR.roughplastic
    for flip, twosided, black in ((True, False, True), (False, False, False), (True, True, False)):
        flat = hostmirror.flatten([DM.plane(hostmirror, make(0.5, 0.7, 1.4896, True, twosided=twosided), flip=flip)], EV.W48, EV.W48, camera=TP.CAM, env=TP.SKY)
        o = open_twin(oracle, packer_constants, flat)
        (xyz, _), t = counted(oracle, lambda: o.sample_pixels(abi.render_params(spp=64, seed=7), EV.crop_pixels()))
        film, _ = o.render(EV.pcg(abi, spp=2, seed=7), threads=8)
        o.close()
        rows = film[EV.CROP[1]:EV.CROP[1] + 8, EV.CROP[0]:EV.CROP[0] + 8, :3]
        assert np.isfinite(xyz).all() and np.isfinite(film).all()
        # (lit: a roughplastic sample can be 0, a dead coat sample beside a next-event direction below the horizon; most are not)
        assert (not xyz.any() and not rows.any()) if black else ((xyz > 0).mean() > 0.9 and (rows > 0).mean() > 0.9)
        assert (t["plastic_from_behind"] >= 64 * 64) == black and (t["plastic_back_face"] > 0) == (flip and twosided), t


def test_c_a_spot_without_a_cone_is_the_point_light(hostmirror, oracle, abi):
    """msk_light_desc: with cos_cutoff = cos_beam = -1 the spot is the point light, to the bit: the films of a plastic box lit by either"""
    prms = WP.identity_params(abi)
    at, inten = (120.0, 420.0, 200.0), (4e5, 3e5, 2e5)
    point = VARIANT_FLATS["plastic"](hostmirror, "lds")
    assert list(point.points[0].position) == list(at)
    spot = hostmirror.flatten(TP.variant_meshes(hostmirror), 48, 48, env=TP.SKY, lights=[SD.spot_spec((278.0, 0.0, 280.0), 40.0, 20.0, origin=at, intensity=inten)])
    spot.lights[0].cos_cutoff = spot.lights[0].cos_beam = -1.0
    o = oracle.scene(point)
    a = [o.render(q, threads=8)[0] for q in prms]
    o.close()
    o = oracle.scene(spot)
    b = [o.render(q, threads=8)[0] for q in prms]
    o.close()
    for x, y in zip(a, b):
        assert np.array_equal(bits(x), bits(y)) and x[..., :3].max() > 0


def with_trailing_plastic(hm, abi, flat, spec):
    """the same scene with one more entry in `bsdfs` that no mesh names"""
    d = flat.desc
    extra = hm._bsdf_desc(hm.MeshSpec("unused", [], 0.5, bsdf=spec), None, d.n_bsdfs)
    arr = (abi.BsdfDesc * (d.n_bsdfs + 1))(*([d.bsdfs[i] for i in range(d.n_bsdfs)] + [extra]))
    flat.keep.append(arr)
    d.bsdfs, d.n_bsdfs = arr, d.n_bsdfs + 1
    return flat


UNUSED_HOSTS = {"point_light": lambda hm: DM.box_flat(hm, "lds", "none"), "mask_and_sky": lambda hm: MB.variant_flat(hm, "lds")}


@pytest.mark.parametrize("host", sorted(UNUSED_HOSTS))
def test_c_an_unused_plastic_entry_changes_nothing(hostmirror, oracle, abi, packer_constants, host):
    """a scene that already holds a point light (or a mask under a `constant` sky) counts the sky with its own density and, with a
    mask, carries the mask records: a plastic entry named by no mesh then changes nothing but the plan, and no bit of the film"""
    prms = WP.identity_params(abi)
    a = twin_films(oracle, packer_constants, UNUSED_HOSTS[host](hostmirror), prms)
    for spec in (TP.plastic(0.4, 0.9, 1.6, True), TR.roughplastic(0.4, 0.9, 1.6, False, 0.2, twosided=True)):
        b = twin_films(oracle, packer_constants, with_trailing_plastic(hostmirror, abi, UNUSED_HOSTS[host](hostmirror), spec), prms)
        for x, y in zip(a, b):
            assert np.array_equal(bits(x), bits(y)) and x[..., :3].max() > 0


def degenerate_box(hm, as_plastic):
    """the Cornell box under a `constant` sky with a point light (the sky then has its own density with or without a plastic); as_plastic:
    every diffuse surface becomes plastic(rho, s = 0, eta = 1)"""
    meshes = hm.cbox_meshes()
    if as_plastic:
        for m in meshes:
            assert m.bsdf is None
            m.bsdf = {"type": "plastic", "diffuse_reflectance": tuple(m.reflectance), "specular_reflectance": 0.0, "int_ior": 1.0, "ext_ior": 1.0, "nonlinear": m.name != "cbox_floor"}
    return hm.flatten(meshes, 32, 32, env=TP.SKY, points=[DM.BOX_POINT])


def test_c_plastic_without_a_coat_at_index_one_is_the_diffuse_bsdf(hostmirror, oracle, abi, packer_constants):
    """plastic(rho, s = 0, eta = 1) in a scene that already counts the sky with its own density: F = 0 (fresnel_dielectric returns 0 for
    eta == 1), fdr_int = 0, ssw = 0 / d_mean = 0, ps = 0 * 0 = 0, pd = 1 * 1 = 1, ps / (ps + pd) = 0 / 1, pd = 1 - 0; D = rho / (1 - 0 *
    rho) or rho / (1 - 0) = rho; f = ((1 * 1) * 1) * 1; eval = ((rho * 1) * (1 / pi)) * cos_o, pdf = 1 * ((1 / pi) * cos_o), value =
    (rho * 1) / 1: every extra operation multiplies or divides by 1 or subtracts 0, which IEEE arithmetic does exactly.  Held on the
    restatement (plastic_ref) against the diffuse BSDF's two expressions, and on the twin's films against the diffuse box's"""
    rng = np.random.RandomState(3)
    n = 2048
    wi = rng.normal(size=(n, 3))
    wi[:, 2] = np.abs(wi[:, 2]) * (rng.uniform(size=n) < 0.9)            # a tenth at cos_i = 0
    wi = (wi / np.linalg.norm(wi, axis=1, keepdims=True)).astype(F)
    hemi = np.array([oracle.warps(u)[2] for u in rng.uniform(0, 1, (n, 2)).astype(F)], F)
    rho = rng.uniform(0, 1, (n, 4)).astype(F)
    for nonlinear in (False, True):
        got = P.sample32(wi, rng.uniform(0, 1, n).astype(F), hemi, rho, np.zeros((n, 4), F), 1.0, F(1), F(0), F(0), nonlinear)
        front = wi[:, 2] > 0
        pdf = np.where(front, (P.INV_PI * hemi[:, 2]).astype(F), F(0))
        assert np.array_equal(got["ok"], front) and not got["delta"].any()
        assert_bits("pdf", got["pdf"], pdf)
        assert_bits("value", got["value"], np.where((pdf > 0)[:, None], rho, F(0)).astype(F))
        ev, ep = P.eval32(wi, hemi, rho, 1.0, F(1), F(0), F(0), nonlinear)
        assert_bits("eval", ev, np.where((front & (hemi[:, 2] > 0))[:, None], ((rho * P.INV_PI).astype(F) * hemi[:, 2:3]).astype(F), F(0)).astype(F))
        assert_bits("eval pdf", ep, np.where(hemi[:, 2] > 0, pdf, F(0)).astype(F))
    prms = WP.identity_params(abi)
    flat = degenerate_box(hostmirror, True)
    o = oracle.scene(flat)
    assert all(o.plastic_constants(b) == (0.0, 0.0) for b in plastic_entries(flat)) and len(plastic_entries(flat)) == flat.desc.n_bsdfs
    o.close()
    a = twin_films(oracle, packer_constants, degenerate_box(hostmirror, False), prms)
    b = twin_films(oracle, packer_constants, flat, prms)
    for x, y in zip(a, b):
        assert np.array_equal(bits(x), bits(y)) and x[..., :3].max() > 0


# ===================================================================================================== (c') refusals
def test_c_the_oracle_refuses_what_the_library_refuses(hostmirror, oracle, abi):
    """type 5, type 8 and beyond, a plastic's ior_eta below 1 or not finite, a specular scale that is not finite, a negative, non-finite or
    unequal alpha on type 7, a back_bsdf out of range: ValueError at scene creation, where a conductor's film came back before;
    `direct` on a scene that holds a plastic: ValueError, as msk_gpu_render_direct answers MSK_ERR_UNSUPPORTED"""
    def make(spec=None):
        return hostmirror.flatten([DM.plane(hostmirror, spec or TP.plastic()), hostmirror.MeshSpec("lamp", [tuple(DM.LAMP)], hostmirror.LUMINAIRE, radiance=(40, 30, 20))],
                                  EV.W48, EV.W48, camera=TP.CAM)
    oracle.scene(make()).close()
    oracle.scene(make(TR.roughplastic())).close()
    inf, nan = float("inf"), float("nan")
    for field, value in (("type", 5), ("type", 8), ("type", 100), ("type", -1), ("ior_eta", 0.99), ("ior_eta", nan), ("ior_eta", inf), ("ior_inv_eta", 0.0),
                         ("back_bsdf", 2), ("back_bsdf", -2)):
        for spec in (TP.plastic(), TR.roughplastic()):
            flat = make(spec)
            setattr(flat.desc.bsdfs[0], field, value)
            with pytest.raises(ValueError):
                oracle.scene(flat)
    for scale in (inf, nan):
        flat = make()
        flat.desc.bsdfs[0].specular_reflectance.scale = scale
        with pytest.raises(ValueError):
            oracle.scene(flat)
    for au, av in ((0.1, 0.2), (-0.1, -0.1), (nan, nan), (inf, inf)):
        flat = make(TR.roughplastic())
        flat.desc.bsdfs[0].alpha_u, flat.desc.bsdfs[0].alpha_v = au, av
        with pytest.raises(ValueError):
            oracle.scene(flat)
        flat = make()                                                    # type 6 does not read alpha
        flat.desc.bsdfs[0].alpha_u, flat.desc.bsdfs[0].alpha_v = au, av
        oracle.scene(flat).close()
    flat = make()                                                        # the lamp's diffuse entry relabelled: refused too, whatever names it
    flat.desc.bsdfs[1].type = 5
    with pytest.raises(ValueError):
        oracle.scene(flat)
    for spec in (TP.plastic(), TR.roughplastic()):
        o = oracle.scene(make(spec))
        prm = abi.render_params(spp=2, seed=1)
        with pytest.raises(ValueError):
            o.render_direct(prm, 1, 1)
        with pytest.raises(ValueError):
            o.sample_pixels_direct(prm, EV.crop_pixels()[:2], 1, 1)
        with pytest.raises(ValueError):
            o.direct_terms(prm, (3, 3), 0, 1, 1)
        assert o.render(prm, threads=2)[0][..., :3].max() > 0            # (`path` renders it)
        o.close()
    # a bare plastic descriptor handed to the BSDF hooks that take no scene has no constants: zeros, not a conductor's values
    bd = make().desc.bsdfs[0]
    val, pdf = oracle.bsdf_eval([bd], 0, (0.3, 0.1, 0.9), (-0.2, 0.4, 0.8))
    wo, spdf, w, eta, typ = oracle.bsdf_sample2([bd], 0, (0.3, 0.1, 0.9), 0.5, (0.3, 0.6))
    assert not val.any() and pdf == 0 and not w.any() and spdf == 0 and typ == 0


# ===================================================================================================== the parity scenes
def all_features_meshes(hm):
    """test_widened_oracle_parity's all-features box with plastics: the floor a roughplastic over the skewed bilinear bitmap (a wide coat,
    alpha 0.7, seen at grazing angles: its mirrored samples often point below the floor); the tall box a nonlinear twosided plastic with
    a checkerboard base; the short box a roughplastic at alpha 1e-4 (the clamp) under the bilinear image mask; the 0.5-masked
    one-sided screen that faces away from the camera a plastic.  The glass ball, the mirror ball, the lamp, the facing screen and the
    masked walls are as there.  One mesh more: a twosided plastic panel before the box that leans back and shows the camera its BACK
    (no closed box is ever met from inside), with a dense coat (eta 2.4) whose mirrored rays leave upwards to the sky: in the films
    with max_depth = 2 only primary hits take a BSDF sample, and this panel is where their coats reach an emitter"""
    meshes = WP.all_features_meshes(hm)
    by = {m.name: m for m in meshes}
    floor, small, big, away = by["cbox_floor"], by["cbox_smallbox"], by["cbox_largebox"], by["screen_away"]
    floor.bsdf = TR.roughplastic(dict(floor.bsdf["texture"]), 1.0, 2.0, True, 0.7)
    big.bsdf = TP.plastic({"type": "checkerboard", "color0": (0.8, 0.2, 0.1), "color1": (0.1, 0.3, 0.7), "scale": (3, 5)}, 0.9, 1.4896, True, twosided=True)
    big.texcoords = [((0, 0), (1, 0), (1, 1), (0, 1)) for _ in big.faces]
    assert small.bsdf["type"] == "mask" and small.bsdf["opacity"]["filter"] == "bilinear"
    small.bsdf = dict(small.bsdf, bsdf=TR.roughplastic((0.3, 0.6, 0.2), 0.8, 1.9, False, 1e-4))
    assert away.bsdf["type"] == "mask" and away.bsdf["opacity"] == 0.5
    away.bsdf = MB.masked(TP.plastic((0.6, 0.5, 0.4), 0.7, 1.3), 0.5)
    for wall, alpha in (("cbox_greenwall", 1.0), ("cbox_redwall", 0.5)):     # the 0.5-masked walls, seen at grazing angles: wide coats under a mask
        assert by[wall].bsdf["type"] == "mask" and by[wall].bsdf["opacity"] == 0.5
        by[wall].bsdf = MB.masked(TR.roughplastic(tuple(by[wall].reflectance), 1.0, 2.2, False, alpha), 0.5)
    x0, x1, yb, zb, yt, zt = 170.0, 350.0, 20.0, -140.0, 158.0, -60.0    # 30 degrees from the vertical; wound so that the normal points away from the camera
    panel = hm.MeshSpec("panel", [((x0, yb, zb), (x1, yb, zb), (x1, yt, zt), (x0, yt, zt))], MB.RHO, bsdf=TP.plastic((0.2, 0.25, 0.3), 1.0, 2.4, True, twosided=True))
    return meshes + [panel]


def all_features_flat(hm, sky, crop=None):
    return hm.flatten(all_features_meshes(hm), 32, 32, env=WP.ALL_SKIES[sky](), points=[WP.ALL_POINT], crop=crop)


_twin_cache = {}


def twin_of_variant(oracle, packer_constants, hm, abi, kind, which):
    """the twin's samples, film, serial film, counters and tallies of a variant scene: computed once, never changed"""
    key = ("variant", kind, which)
    if key not in _twin_cache:
        flat = VARIANT_FLATS[kind](hm, which)
        o = open_twin(oracle, packer_constants, flat)
        p_xyz, p_film, p_serial = WP.variant_params(abi)
        (xyz, pos), _ = counted(oracle, lambda: sample_pixels_threaded(o, p_xyz, EV.crop_pixels()))
        (film, st), tally = counted(oracle, lambda: o.render(p_film, threads=8))
        (serial, sst), stally = counted(oracle, lambda: o.render(p_serial, threads=8))
        consts = {b: o.plastic_constants(b) for b in plastic_entries(flat)}
        o.close()
        for a in (xyz, pos, film, serial):
            a.setflags(write=False)
        _twin_cache[key] = dict(flat=flat, xyz=xyz, pos=pos, film=film, serial=serial, st=(st.samples, st.segments), tally=tally,
                                sst=(sst.samples, sst.segments), stally=stally, consts=consts)
    return _twin_cache[key]


def twin_of_all_features(oracle, packer_constants, hm, abi, sky):
    key = ("all", sky)
    if key not in _twin_cache:
        o = open_twin(oracle, packer_constants, all_features_flat(hm, sky))
        out = []
        for prm in WP.all_features_params(abi):
            (film, st), tally = counted(oracle, lambda: o.render(prm, threads=8))
            film.setflags(write=False)
            out.append(dict(film=film, st=(st.samples, st.segments), tally=tally))
        o.close()
        _twin_cache[key] = out
    return _twin_cache[key]


# ===================================================================================================== (d) coverage
NEW = set(oracle_binding.Oracle.PATH_TALLIES[15:25])                   # the plastics' ten (what was appended later belongs to test_lens_light_oracle_parity)
EVERY = WP.EVERY | NEW
SMOOTH_T = {"plastic_coat", "plastic_base", "emitter_after_coat"}
ROUGH_T = {"roughplastic_coat", "roughplastic_base", "roughplastic_failed"}
# The variant scenes (test_plastic_bsdf.variant_meshes): a `constant` sky, a point light, an area lamp, a bitmap floor, a glass ball; the
# tall box a twosided plastic, the short box one-sided.  No mask, hide_emitters off, rr_depth 5.  These scenes and their parameters
# belong to the `variant_reference` fixtures and are not shaped here, so three branches stay below 100 in their 8-spp film and are
# neither required nor impossible (the all-features scene below is shaped to reach them in every film):
#   rr_after_coat         54 .. 58: Russian roulette starts at the fourth bounce here, and a coat is one sample in seven
#   roughplastic_failed   49: alpha 0.05 and 0.1, two narrow coats whose mirrored direction seldom points below the surface
#   plastic_from_behind / plastic_back_face   0 for the smooth plastic, 39 / 16 for the rough one, whose vertex-free boxes are met from
#                         inside only by rays that a dead coat sample sent below the surface
VARIANT_COVERAGE = {
    "plastic": dict(meant=SMOOTH_T | {"sky_own_density", "emitter_after_delta", "point_unoccluded", "point_occluded", "texel_wrap"},
                    cannot=ROUGH_T | WP.NULL_T | {"null_over_plastic", "envmap_miss_after_smooth", "envmap_pole_clamp"}),
    "roughplastic": dict(meant=(ROUGH_T - {"roughplastic_failed"}) | {"sky_own_density", "emitter_after_delta", "point_unoccluded", "point_occluded", "texel_wrap"},
                         cannot=SMOOTH_T | WP.NULL_T | {"null_over_plastic", "envmap_miss_after_smooth", "envmap_pole_clamp"}),
}
VARIANT_IDS = [(kind, which) for kind in sorted(VARIANT_FLATS) for which in ("lds", "hbm")]


@pytest.mark.parametrize("kind,which", VARIANT_IDS)
def test_d_variant_scenes_reach_their_branches(hostmirror, oracle, abi, packer_constants, kind, which):
    run = twin_of_variant(oracle, packer_constants, hostmirror, abi, kind, which)
    cov = VARIANT_COVERAGE[kind]
    assert cov["meant"] | cov["cannot"] <= EVERY and not cov["meant"] & cov["cannot"]
    t = run["tally"]
    print("TALLY %s %s film: %s" % (kind, which, t))
    print("TALLY %s %s serial film: %s" % (kind, which, run["stally"]))
    for k in sorted(cov["meant"]):
        assert t[k] >= 100, (kind, which, k, t)
        assert run["stally"][k] >= 1, (kind, which, k, run["stally"])
    for k in sorted(cov["cannot"]):
        assert t[k] == 0 and run["stally"][k] == 0, (kind, which, k, t)


def all_features_coverage(abi, sky, prm):
    """(meant, cannot) of ONE film of the grid: test_widened_oracle_parity's rule for the eleven earlier events, and for the plastics'
    ten: Russian roulette runs only in the films with rr_depth = 2; everything else is meant in every film"""
    meant, cannot = WP.all_features_coverage(abi, sky, prm)
    cannot = set(cannot)
    if prm.rr_depth != 2:
        cannot |= {"rr_after_coat"}
    return (set(meant) | NEW) - cannot, cannot


@pytest.mark.parametrize("sky", sorted(WP.ALL_SKIES))
def test_d_the_all_features_scene_reaches_every_branch(hostmirror, oracle, abi, packer_constants, sky):
    """PER FILM, as test_widened_oracle_parity's (d) and for its reason.  Every counter-RNG film (8 spp) reaches each of its meant
    tallies at least 100 times on its own; the 2-spp MSK_RNG_PCG_BLOCK films at least once; what a film cannot produce is 0"""
    runs = twin_of_all_features(oracle, packer_constants, hostmirror, abi, sky)
    for prm, run in zip(WP.all_features_params(abi), runs):
        t = run["tally"]
        what = "all-features-plastic %s rng %d hide %d max_depth %d rr_depth %d" % (sky, prm.rng_mode, prm.hide_emitters, prm.max_depth, prm.rr_depth)
        print("TALLY %s: %s" % (what, t))
        meant, cannot = all_features_coverage(abi, sky, prm)
        assert meant | cannot == EVERY
        for k in sorted(meant):
            assert t[k] >= (100 if prm.rng_mode == abi.MSK_RNG_COUNTER else 1), (what, k, t)
        for k in sorted(cannot):
            assert t[k] == 0, (what, k, t)


# ===================================================================================================== GPU layer
@pytest.mark.gpu
@pytest.mark.parametrize("kind,which", VARIANT_IDS)
def test_e_default_configuration_equals_the_twin(gpu_ctx, hostmirror, oracle, abi, packer_constants, monkeypatch, kind, which):
    """the scenes and parameters of the `variant_reference` fixtures of test_plastic_bsdf / test_roughplastic_bsdf: this one hop ties every
    execution variant and tree form those files hold to their default to the oracle"""
    WP.no_knobs(monkeypatch)
    want = twin_of_variant(oracle, packer_constants, hostmirror, abi, kind, which)
    p_xyz, p_film, p_serial = WP.variant_params(abi)
    g = abi.Scene(gpu_ctx, want["flat"])
    try:
        for b, k in want["consts"].items():
            assert np.array_equal(bits(np.array(g.plastic_constants(b))), bits(np.array(k))), (kind, which, b, g.plastic_constants(b), k)
        xyz, pos = g.sample_pixels(p_xyz, EV.crop_pixels())
        film, st = g.render(p_film)
        serial, sst = g.render(p_serial)
    finally:
        g.close()
    assert len(want["consts"]) == 2
    assert np.array_equal(bits(pos), bits(want["pos"])), (kind, which)
    bad = (bits(xyz) != bits(want["xyz"])).any(-1)
    assert not bad.any(), (kind, which, int(bad.sum()), np.argwhere(bad)[:4].tolist(), xyz[bad][:3], want["xyz"][bad][:3])
    assert np.array_equal(bits(film), bits(want["film"])), (kind, which, int((bits(film) != bits(want["film"])).sum()), float(np.abs(film - want["film"]).max()))
    assert np.array_equal(bits(serial), bits(want["serial"])), (kind, which, int((bits(serial) != bits(want["serial"])).sum()))
    check_counters("%s %s film" % (kind, which), st, want["st"], want["tally"], p_film.rng_mode, abi)
    check_counters("%s %s serial film" % (kind, which), sst, want["sst"], want["stally"], p_serial.rng_mode, abi)


@pytest.mark.gpu
@pytest.mark.parametrize("placement", ["default", "hbm"])
@pytest.mark.parametrize("sky", sorted(WP.ALL_SKIES))
def test_f_all_features_scene_equals_the_twin(gpu_ctx, hostmirror, oracle, abi, packer_constants, monkeypatch, sky, placement):
    WP.no_knobs(monkeypatch, **({"MSK_LDS_SCENE_KB": "0"} if placement == "hbm" else {}))
    runs = twin_of_all_features(oracle, packer_constants, hostmirror, abi, sky)
    g = abi.Scene(gpu_ctx, all_features_flat(hostmirror, sky))
    try:
        for prm, want in zip(WP.all_features_params(abi), runs):
            film, st = g.render(prm)
            what = "all-features-plastic %s %s rng %d hide %d max_depth %d rr_depth %d" % (sky, placement, prm.rng_mode, prm.hide_emitters, prm.max_depth, prm.rr_depth)
            assert np.array_equal(bits(film), bits(want["film"])), (what, int((bits(film) != bits(want["film"])).sum()), float(np.abs(film - want["film"]).max()))
            assert film[..., :3].max() > 0
            check_counters(what, st, want["st"], want["tally"], prm.rng_mode, abi)
    finally:
        g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("sky", sorted(WP.ALL_SKIES))
def test_f_crop_window_shards_and_samples(gpu_ctx, hostmirror, oracle, abi, packer_constants, monkeypatch, sky):
    """a crop window (both RNG modes); the two sample shards (0, 2) and (1, 2), each against the twin's film of the same shard; and
    the samples of every pixel at spp 4"""
    WP.no_knobs(monkeypatch)
    crop = (5, 3, 20, 18)
    prms = [abi.render_params(spp=8, seed=5, rr_depth=2), EV.pcg(abi, spp=2, seed=5, rr_depth=2)]
    o, g = open_twin(oracle, packer_constants, all_features_flat(hostmirror, sky, crop=crop)), abi.Scene(gpu_ctx, all_features_flat(hostmirror, sky, crop=crop))
    try:
        for prm in prms:
            film, st = g.render(prm)
            ref, rst = o.render(prm, threads=8)
            assert film.shape == ref.shape == (18, 20, 5) and st.samples == rst.samples
            assert np.array_equal(bits(film), bits(ref)), (sky, prm.rng_mode, int((bits(film) != bits(ref)).sum()))
    finally:
        g.close(); o.close()
    o, g = open_twin(oracle, packer_constants, all_features_flat(hostmirror, sky)), abi.Scene(gpu_ctx, all_features_flat(hostmirror, sky))
    try:
        for r in (0, 1):
            prm = abi.render_params(spp=8, seed=5, rr_depth=2, sample_first=r, sample_stride=2)
            film, st = g.render(prm)
            ref, rst = o.render(prm, threads=8)
            assert st.samples == rst.samples == 32 * 32 * 4
            assert np.array_equal(bits(film), bits(ref)), (sky, r, int((bits(film) != bits(ref)).sum()))
        px = np.array([(x, y) for y in range(32) for x in range(32)], np.int32)
        prm = abi.render_params(spp=4, seed=5, rr_depth=2, hide_emitters=1)
        xyz, pos = g.sample_pixels(prm, px)
        rxyz, rpos = sample_pixels_threaded(o, prm, px)
        assert np.array_equal(bits(pos), bits(rpos))
        bad = (bits(xyz) != bits(rxyz)).any(-1)
        assert not bad.any(), (sky, int(bad.sum()), np.argwhere(bad)[:4].tolist(), xyz[bad][:3], rxyz[bad][:3])
    finally:
        g.close(); o.close()


@pytest.mark.gpu
def test_g_aov_on_the_plastic_scene_equals_the_twin(gpu_ctx, hostmirror, oracle, abi, packer_constants, monkeypatch):
    """every channel of an "aov" render with the nested path integrator on the plastic variant scene"""
    WP.no_knobs(monkeypatch)
    flat = twin_of_variant(oracle, packer_constants, hostmirror, abi, "plastic", "lds")["flat"]
    types = [abi.MSK_AOV_DEPTH, abi.MSK_AOV_POSITION, abi.MSK_AOV_UV, abi.MSK_AOV_GEO_NORMAL, abi.MSK_AOV_SH_NORMAL, abi.MSK_AOV_PATH_RGBA]
    prm = abi.render_params(spp=4, seed=5)
    o, g = oracle.scene(flat), abi.Scene(gpu_ctx, flat)
    try:
        for t in (types, types[:5]):
            film, st = g.render_aov(prm, t)
            ref, rst = o.render_aov(prm, t, threads=8)
            assert film.shape == ref.shape and st.samples == rst.samples
            for c in range(film.shape[-1]):
                assert np.array_equal(bits(film[..., c]), bits(ref[..., c])), (len(t), c, int((bits(film[..., c]) != bits(ref[..., c])).sum()))
        assert np.abs(ref[..., 5:]).max() > 0
    finally:
        g.close(); o.close()
