"""Randomised parity: triangle soups with slivers, every BSDF type with random parameters, one to three area emitters,
optional environment, random integrator properties and block sizes (tools/fuzz_parity.py; 4300 such scenes were run
bit-identical during development) — a slice of it as a regression test."""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fuzz():
    spec = importlib.util.spec_from_file_location("fuzz_parity", os.path.join(ROOT, "tools", "fuzz_parity.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_random_scenes_are_valid_oracle_inputs(oracle, abi):
    """CPU: the generator produces scenes the oracle renders to finite films, deterministically per seed."""
    fz = _fuzz()
    for s in (1, 2, 3):
        flat = fz.random_scene(np.random.RandomState(s))
        sc = oracle.scene(flat)
        a, _ = sc.render(abi.render_params(spp=2, seed=s), threads=2)
        b, _ = sc.render(abi.render_params(spp=2, seed=s), threads=3)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and np.isfinite(a[..., 4]).all() and a[..., 4].min() > 0
        sc.close()
    # with the smooth `dielectric` on some meshes (glass=True): valid inputs as well, at least one glass BSDF per scene, and the
    # scene without the option is unchanged by its existence (the choice is drawn from a generator of its own)
    for s in (9001, 9005, 9006, 9007):
        flat = fz.random_scene(np.random.RandomState(s), glass=True, seed=s)
        plain, again = fz.random_scene(np.random.RandomState(s)), fz.random_scene(np.random.RandomState(s), glass=False, seed=s)
        d = flat.desc
        assert any(d.bsdfs[i].type == abi.MSK_BSDF_DIELECTRIC for i in range(d.n_bsdfs))
        assert not any(plain.desc.bsdfs[i].type == abi.MSK_BSDF_DIELECTRIC for i in range(plain.desc.n_bsdfs))
        assert np.array_equal(flat.vertices.view(np.uint32), plain.vertices.view(np.uint32)) and np.array_equal(flat.faces, plain.faces)
        assert np.array_equal(again.vertices.view(np.uint32), plain.vertices.view(np.uint32))
        assert all(bytes(again.desc.bsdfs[i]) == bytes(plain.desc.bsdfs[i]) for i in range(plain.desc.n_bsdfs))
        sc = oracle.scene(flat)
        a, st = sc.render(abi.render_params(spp=2, seed=s), threads=2)
        b, _ = sc.render(abi.render_params(spp=2, seed=s), threads=3)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and np.isfinite(a).all() and a[..., 4].min() > 0 and st.invalid_samples == 0
        sc.close()
    # with `plastic` / `roughplastic` on some meshes (plastic=True): the same three properties, and both types occur over the seeds
    seen = set()
    for s in (11001, 11002, 11005, 11006):                              # (11007 draws an extrapolated table that goes negative, with or without plastics)
        flat = fz.random_scene(np.random.RandomState(s), plastic=True, seed=s)
        plain, again = fz.random_scene(np.random.RandomState(s)), fz.random_scene(np.random.RandomState(s), plastic=False, seed=s)
        d = flat.desc
        types = {d.bsdfs[i].type for i in range(d.n_bsdfs)}
        assert types & {abi.MSK_BSDF_PLASTIC, abi.MSK_BSDF_ROUGHPLASTIC}
        seen |= types
        assert not any(plain.desc.bsdfs[i].type in (abi.MSK_BSDF_PLASTIC, abi.MSK_BSDF_ROUGHPLASTIC) for i in range(plain.desc.n_bsdfs))
        assert np.array_equal(flat.vertices.view(np.uint32), plain.vertices.view(np.uint32)) and np.array_equal(flat.faces, plain.faces)
        assert np.array_equal(again.vertices.view(np.uint32), plain.vertices.view(np.uint32))
        assert all(bytes(again.desc.bsdfs[i]) == bytes(plain.desc.bsdfs[i]) for i in range(plain.desc.n_bsdfs))
        sc = oracle.scene(flat)
        a, st = sc.render(abi.render_params(spp=2, seed=s), threads=2)
        b, _ = sc.render(abi.render_params(spp=2, seed=s), threads=3)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and np.isfinite(a).all() and a[..., 4].min() > 0 and st.invalid_samples == 0
        sc.close()
    assert {abi.MSK_BSDF_PLASTIC, abi.MSK_BSDF_ROUGHPLASTIC} <= seen
    # with a `thinlens` sensor (lens=True) and with `spot` / `directional` emitters (lights=True): valid inputs, the option is in the
    # scene, and nothing else of the scene moved: the lens leaves every byte of the flat as it was, the lights append emitters behind
    # the scene's own.  A lens scene is refused under MSK_RNG_PCG_BLOCK.  Apertures of 0 and above, spots and suns occur over the seeds
    radii, kinds = set(), set()
    for s in (13001, 13003, 13004, 13005):                              # (13002 draws a table whose extrapolation goes negative: its film's minimum is
                                                                        # below 0 with or without a lens, and through the lens three samples in 2^18 pass -1e-5)
        plain = fz.random_scene(np.random.RandomState(s))
        for opt in (dict(lens=True), dict(lights=True), dict(lens=True, lights=True)):
            flat = fz.random_scene(np.random.RandomState(s), seed=s, **opt)
            d, pd = flat.desc, plain.desc
            assert (flat.lens is not None) == ("lens" in opt) and (flat.lights is not None) == ("lights" in opt) and plain.lens is None and plain.lights is None
            assert np.array_equal(flat.vertices.view(np.uint32), plain.vertices.view(np.uint32)) and np.array_equal(flat.faces, plain.faces)
            assert bytes(d.camera) == bytes(pd.camera) and bytes(d.film) == bytes(pd.film) and d.n_bsdfs == pd.n_bsdfs
            assert all(bytes(d.bsdfs[i]) == bytes(pd.bsdfs[i]) for i in range(pd.n_bsdfs)) and all(bytes(d.emitters[i]) == bytes(pd.emitters[i]) for i in range(pd.n_emitters))
            if "lights" in opt:
                extra = [d.emitters[i].type for i in range(pd.n_emitters, d.n_emitters)]
                assert 1 <= len(extra) <= 3 and set(extra) <= {abi.MSK_EMITTER_SPOT, abi.MSK_EMITTER_DIRECTIONAL} and len(flat.lights) == len(extra)
                kinds |= set(extra)
            else:
                assert fz.scene_digest(flat) == fz.scene_digest(plain)
            if "lens" in opt:
                radii.add(flat.lens.aperture_radius > 0)
            sc = oracle.scene(flat)
            assert (sc.lens is not None) == ("lens" in opt)
            a, st = sc.render(abi.render_params(spp=2, seed=s), threads=2)
            b, _ = sc.render(abi.render_params(spp=2, seed=s), threads=3)
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and np.isfinite(a).all() and a[..., 4].min() > 0 and st.invalid_samples == 0
            if "lens" in opt:
                with pytest.raises(ValueError):
                    sc.render(abi.render_params(spp=2, seed=s, rng_mode=abi.MSK_RNG_PCG_BLOCK), threads=2)
            sc.close()
    assert radii == {False, True} and kinds == {abi.MSK_EMITTER_SPOT, abi.MSK_EMITTER_DIRECTIONAL}


def test_the_seeds_of_the_regression_sweeps_still_make_their_scenes():
    """The scenes of the seeds the GPU sweeps below use (5000-5060, 7000-7007, 20657), as digests recorded before the generator
    learnt the glass option (tests/golden/fuzz_scene_digests.json): an option added to random_scene must not move them."""
    import json
    fz = _fuzz()
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "fuzz_scene_digests.json")))
    assert sorted(int(k) for k in want) == list(range(5000, 5061)) + list(range(7000, 7008)) + [20657]
    moved = [int(k) for k, v in want.items() if fz.scene_digest(fz.random_scene(np.random.RandomState(int(k)))) != v]
    assert moved == []
    # ... nor the lens and the spot / sun options: switched off by name, and the lens switched on (it is no part of the flat's
    # bytes), three kept seeds still make the recorded bytes
    for k in (5000, 7003, 20657):
        for opt in (dict(lens=False, lights=False), dict(lens=True)):
            assert fz.scene_digest(fz.random_scene(np.random.RandomState(k), seed=k, **opt)) == want[str(k)], (k, opt)


def test_hit_acceptance_does_not_depend_on_the_tree(oracle):
    """Oracle deviation D10, found by this sweep (seed 20657): a shadow ray lying in the plane of a sliver emitter triangle
    gets a numerical Moeller-Trumbore "hit" 40 units outside the triangle (float64: u = -0.13), which a tree reports or
    culls depending on its leaves.  With the bounds predicate brute force and the BVH agree — on this ray and on random
    rays through random sliver soups."""
    import json
    fz = _fuzz()
    fixture = json.load(open(os.path.join(ROOT, "tests", "golden", "d10_scene.json")))
    soup = fz.hm.MeshSpec("soup", [tuple(tuple(v) for v in t) for t in fixture["triangles"]], (0.5, 0.5, 0.5), radiance=(1, 1, 1))
    sc = oracle.scene(fz.hm.flatten([soup], 16, 16))
    ray = np.array([fixture["ray"]], np.float32)
    # without the bounds predicate the Moeller-Trumbore arithmetic alone reports t = 204.8 on triangle 0 (checked when the
    # fixture was made); with it nothing is hit, with or without the tree
    with_bvh = (sc.trace_any(ray).copy(), sc.trace_closest(ray).copy())
    sc.set_bvh(0)
    assert np.array_equal(sc.trace_any(ray), with_bvh[0]) and with_bvh[0][0] == 0
    assert np.array_equal(sc.trace_closest(ray).view(np.uint32), with_bvh[1].view(np.uint32))
    sc.close()
    rng = np.random.RandomState(7)
    for s in (20657, 11, 12, 13):
        sc = oracle.scene(fz.random_scene(np.random.RandomState(s)))
        o = rng.uniform(-600, 900, (4000, 3)); d = rng.normal(size=(4000, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
        # a third of the rays lie (almost) in the plane z = const through their origin: the near-parallel regime
        d[::3, 2] *= 1e-7
        rays = np.concatenate([o, np.full((4000, 1), 1e-3), d, np.full((4000, 1), 3000.0)], 1).astype(np.float32)
        sc.set_bvh(1)
        a = sc.trace_closest(rays).copy(); occ = sc.trace_any(rays).copy()
        sc.set_bvh(0)
        assert np.array_equal(sc.trace_closest(rays).view(np.uint32), a.view(np.uint32)) and np.array_equal(sc.trace_any(rays), occ)
        sc.close()


@pytest.mark.gpu
def test_gpu_equals_oracle_on_random_scenes(gpu_ctx, oracle):
    assert _fuzz().sweep(gpu_ctx, oracle, list(range(5000, 5060)) + [20657]) == []


@pytest.mark.gpu
def test_gpu_equals_oracle_on_random_scenes_with_many_samples(gpu_ctx, oracle):
    """The same random scenes at 400 spp: enough samples (>= 1024 regions) for the wavefront loop to run as four loops on
    four streams with every material, emitter and shard kind the generator makes."""
    assert _fuzz().sweep(gpu_ctx, oracle, list(range(7000, 7008)), verbose=False, spp=400) == []


@pytest.mark.gpu
def test_gpu_equals_oracle_on_random_scenes_with_glass(gpu_ctx, oracle):
    """The sweep with some meshes of every scene turned into the smooth `dielectric` (either side dense, tinted, some of them
    emitters), next to whatever else the generator makes"""
    assert _fuzz().sweep(gpu_ctx, oracle, list(range(9000, 9040)), glass=True) == []


@pytest.mark.gpu
def test_gpu_equals_oracle_on_random_scenes_with_glass_and_many_samples(gpu_ctx, oracle):
    assert _fuzz().sweep(gpu_ctx, oracle, list(range(9100, 9104)), verbose=False, spp=400, glass=True) == []


@pytest.mark.gpu
def test_gpu_equals_oracle_on_random_scenes_with_plastic(gpu_ctx, oracle):
    """The sweep with some meshes of every scene turned into `plastic` or `roughplastic` (any relative index from 1 up, either base
    formula, coats from alpha 1e-4 to 0.5, textured and tabulated spectra, one- and twosided, some under a mask, some of them
    emitters), next to whatever else the generator makes"""
    assert _fuzz().sweep(gpu_ctx, oracle, list(range(11000, 11040)), plastic=True) == []


@pytest.mark.gpu
def test_gpu_equals_oracle_on_random_scenes_with_plastic_and_many_samples(gpu_ctx, oracle):
    assert _fuzz().sweep(gpu_ctx, oracle, list(range(11100, 11104)), verbose=False, spp=400, plastic=True) == []


@pytest.mark.gpu
def test_gpu_equals_oracle_on_random_scenes_with_a_lens(gpu_ctx, oracle):
    """The sweep through a `thinlens` sensor (an aperture that is 0, small or as wide as the scene, focused before, inside or behind
    it): the `_l` kernels with whatever else the generator makes, ragged films, crop windows and shards included"""
    assert _fuzz().sweep(gpu_ctx, oracle, list(range(13000, 13040)), lens=True) == []


@pytest.mark.gpu
def test_gpu_equals_oracle_on_random_scenes_with_spots_and_suns(gpu_ctx, oracle):
    """The sweep with one to three `spot` / `directional` emitters behind the scene's own; the second half of the seeds through a
    lens as well, with plastics on some meshes: everything the `_l` kernels carry"""
    fz = _fuzz()
    assert fz.sweep(gpu_ctx, oracle, list(range(15000, 15020)), lights=True) == []
    assert fz.sweep(gpu_ctx, oracle, list(range(15020, 15040)), lights=True, lens=True, plastic=True) == []


def _fuzz_rays():
    spec = importlib.util.spec_from_file_location("fuzz_rays", os.path.join(ROOT, "tools", "fuzz_rays.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.gpu
def test_adversarial_rays_gpu_equals_oracle_brute_force(gpu_ctx, oracle, abi):
    """Rays from vertices / edges / planes of the triangles towards other vertices, along edges, axis-aligned, with tmax
    exactly at the target (tools/fuzz_rays.py; 5 M such rays identical in development, after it had found that the GPU
    dropped first hits whose t exceeds tmax by an ulp): whatever tree the GPU uses vs the oracle's brute force."""
    fr = _fuzz_rays()
    for s in (3, 4, 5, 143):
        rng = np.random.RandomState(s)
        flat = fr.fz.random_scene(rng)
        d = flat.desc
        tris = np.array([[flat.vertices[d.meshes[m].first_vertex + i, :3] for i in flat.faces[f]] for m in range(d.n_meshes)
                         for f in range(d.meshes[m].first_face, d.meshes[m].first_face + d.meshes[m].face_count)], np.float32)
        rays = fr.adversarial_rays(rng, tris, 20000)
        g, o = abi.Scene(gpu_ctx, flat), oracle.scene(flat)
        o.set_bvh(0)
        assert np.array_equal(g.trace_closest(rays).view(np.uint32), o.trace_closest(rays).view(np.uint32)), s
        assert np.array_equal(g.trace_any(rays), o.trace_any(rays)), s
        g.close()
        o.close()


@pytest.mark.gpu
@pytest.mark.parametrize("offset", [1e5, -3e5])
def test_adversarial_rays_on_a_scene_far_from_the_origin(gpu_ctx, oracle, abi, offset):
    """The same sweep on scenes translated away from the origin, where an ulp of a coordinate (0.008 at 1e5) is no longer small
    against the scene's extent: the padding of the boxes and of the D10 bounds follows the scene's SCALE = max(diagonal, largest
    |coordinate|) (tests/test_padding_margin.py), so the LDS-resident binary tree (seed 3) and the quantised 4-wide tree in HBM
    (seed 4: 4.5 k triangles) still give the brute-force answer bit for bit."""
    fr = _fuzz_rays()
    for s in (3, 4):
        rng = np.random.RandomState(s)
        flat = fr.fz.random_scene(rng)
        flat.vertices[:, :3] += np.float32(offset)
        d = flat.desc
        tris = np.array([[flat.vertices[d.meshes[m].first_vertex + i, :3] for i in flat.faces[f]] for m in range(d.n_meshes)
                         for f in range(d.meshes[m].first_face, d.meshes[m].first_face + d.meshes[m].face_count)], np.float32)
        rays = fr.adversarial_rays(rng, tris, 20000)
        g, o = abi.Scene(gpu_ctx, flat), oracle.scene(flat)
        o.set_bvh(0)
        assert np.array_equal(g.trace_closest(rays).view(np.uint32), o.trace_closest(rays).view(np.uint32)), s
        assert np.array_equal(g.trace_any(rays), o.trace_any(rays)), s
        g.close()
        o.close()


@pytest.mark.gpu
def test_gpu_trees_equal_brute_force_with_a_tenth_of_the_padding(gpu_ctx, oracle, abi, monkeypatch):
    """The margin of the padding rule for the DEVICE's slab arithmetic (v_rcp_f32 reciprocals, `plane * idir - o * idir`, the
    quantised nodes' decode): with MSK_PAD_SCALE=1e-6 on both sides — a tenth of the rule's padding — the LDS-resident binary tree
    (seeds 3, 5), the quantised 4-wide tree in HBM (seeds 0, 4) and the same scenes 1e5 units from the origin still give the oracle's
    brute-force answer on adversarial rays, bit for bit (the CPU counterpart: tests/test_padding_margin.py)."""
    monkeypatch.setenv("MSK_PAD_SCALE", "1e-6")
    fr = _fuzz_rays()
    for s, offset in ((3, 0.0), (0, 0.0), (4, 0.0), (5, 1e5), (4, 1e5)):
        rng = np.random.RandomState(s)
        flat = fr.fz.random_scene(rng)
        if offset:
            flat.vertices[:, :3] += np.float32(offset)
        d = flat.desc
        tris = np.array([[flat.vertices[d.meshes[m].first_vertex + i, :3] for i in flat.faces[f]] for m in range(d.n_meshes)
                         for f in range(d.meshes[m].first_face, d.meshes[m].first_face + d.meshes[m].face_count)], np.float32)
        rays = fr.adversarial_rays(rng, tris, 20000)
        g, o = abi.Scene(gpu_ctx, flat), oracle.scene(flat)
        o.set_bvh(0)
        assert np.array_equal(g.trace_closest(rays).view(np.uint32), o.trace_closest(rays).view(np.uint32)), (s, offset)
        assert np.array_equal(g.trace_any(rays), o.trace_any(rays)), (s, offset)
        g.close()
        o.close()


@pytest.mark.gpu
@pytest.mark.parametrize("bad", ["0", "abc", "-1e-5", "nan", "1", "1e-9", ""])
def test_a_padding_knob_that_is_not_a_sane_number_is_refused(gpu_ctx, abi, hostmirror, golden_lookup, monkeypatch, bad):
    """MSK_PAD_SCALE is honoured for the margin tests only within [1e-7, 1e-3]: zero, garbage or a stray value would silently take
    the padding out of the GPU library AND the oracle at once — the parity tests would still pass (round 4's advisor finding)."""
    monkeypatch.setenv("MSK_PAD_SCALE", bad)
    with pytest.raises(abi.MskError) as e:
        abi.Scene(gpu_ctx, hostmirror.cbox_scene(16, 16, coeff_lookup=golden_lookup))
    assert e.value.code == abi.MSK_ERR_INVALID_ARG and "MSK_PAD_SCALE" in str(e.value)
