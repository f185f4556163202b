"""Scenes whose shading tables do not fit in LDS: every branch of how msk_gpu_scene_create and msk_gpu_render place them.

The placement moves data and never changes arithmetic, so every scene here must give the oracle's bits.  The plan makes four
decisions (misaki-render_amd/csrc/msk_plan.h: place_tree and place_tables at scene creation, make_launch_plan per render;
msk_kernels.h: stage_tables and its callers):

  tree      BVH and triangles in LDS (trace mode 0, k_trace_q) or in HBM (mode 6); pinned per scene with MSK_LDS_SCENE_KB
  tables    table_f4 <= 2560 float4: every shading table in LDS (k_shade_gen<true, ...>), else only the small ones (<false, ...>)
  staged    small_f4 <= 1024 float4: stage_tables<false> copies the small tables to LDS, else it takes its HBM branch
  fused     k_wavefront (tree and tables in LDS) or k_wavefront_h (both in HBM) for the thin end of a pass; MSK_FUSED=1 runs
            the whole pass there.  The one decision a test can observe: msk_stats::launches_wavefront.

The CPU tests pin each scene to its named side with table_plan (the library's formulas) and check the oracle on it; the GPU
tests compare films, sample records and the other entry points with the oracle bit for bit.  GPU tests need an MI355X."""
import functools
import time

import numpy as np
import pytest

W, H, SPP, SEED = 96, 80, 8, 5
ORACLE_THREADS = 16
LDS_TABLES_F4 = 40 * 1024 // 16          # msk_plan.h: kLdsTablesLimit (place_tables: lds_tables = table_bytes <= 40 KB)
SMALL_TABLES_F4 = 16 * 1024 // 16        # msk_layout.h: MSK_SMALL_TABLES_KB (default 16)


def table_plan(flat):
    """table_f4, small_f4 and the two decisions they make, from the msk_scene_desc alone.  Mirrors `table_bytes`,
    `small_bytes` and `place_tables` of misaki-render_amd/csrc/msk_plan.h — tests/test_scene_tables.py holds this function
    against them on a CPU — and tables_lds_float4s / small_tables_float4s (msk_kernels.h, next to stage_tables), with the
    counts as msk_scene_tables.h packs them.  In float4: mesh records (1 each), BSDF
    records (7 each, at least one) and texture records (3 each), emitter records (2) and grids (1), the emitters' 95-entry D65
    tables, the concatenated area CDFs (face_count + 1 per area emitter, at least one entry), the CIE table (285 floats = 72)
    and the tabulated spectra's values.  table_f4 adds tri_verts and tri_frames, 6 per triangle."""
    d = flat.desc
    ems = [d.emitters[i] for i in range(d.n_emitters)]
    cdf_len = sum(d.meshes[e.mesh_id].face_count + 1 for e in ems if e.mesh_id >= 0) or 1
    n_bsdf_f4 = max(1, d.n_bsdfs) * 7 + 3 * d.n_textures
    small = (d.n_meshes + n_bsdf_f4 + 3 * d.n_emitters + (95 * d.n_emitters + 3) // 4 + (cdf_len + 3) // 4 + 72 +
             (d.n_regular_values + 3) // 4)
    table = 6 * d.n_faces + small
    return dict(table_f4=table, small_f4=small, lds_tables=table <= LDS_TABLES_F4, small_staged=small <= SMALL_TABLES_F4)


# ----------------------------------------------------------------------------- scene pieces
def ceiling_quad(hm, name, x, z, half, radiance, y=545.0):
    """a small square facing down, wound like the cbox luminaire (it emits towards the floor)"""
    q = ((x + half, y, z - half), (x + half, y, z + half), (x - half, y, z + half), (x - half, y, z - half))
    return hm.MeshSpec(name, [q], hm.LUMINAIRE, radiance=radiance)


def ceiling_quads(hm, n, half, radiance, tag):
    """n emissive squares on a grid under the ceiling, clear of the luminaire"""
    k = int(np.ceil(np.sqrt(n * 1.25))) + 1
    out = []
    for z in np.linspace(30, 530, k):
        for x in np.linspace(30, 526, k):
            if 200 <= x <= 356 and 214 <= z <= 345:
                continue
            out.append(ceiling_quad(hm, f"{tag}{len(out)}", float(x), float(z), half, radiance))
            if len(out) == n:
                return out
    raise AssertionError(n)


def zero_area_emitter(hm):
    """an emitter whose two faces have no area: its CDF is 0 * (1 / 0) = NaN and its pdf 1 / 0, as in the reference"""
    p = (150.0, 545.0, 150.0)
    return hm.MeshSpec("zero_area_lamp", [(p, p, p, p)], hm.LUMINAIRE, radiance=(5, 5, 5))


def faceless_pads(hm, delta):
    """meshes without faces that add exactly `delta` float4 to small_f4 (and so to table_f4): a plain one costs a mesh
    record and a BSDF record (1 + 7), a checkerboard-textured one 3 more (its texture record)"""
    b = (3 * delta) % 8                          # 8 a + 11 b = delta  (11 * 3 = 33 = 1 mod 8)
    a = (delta - 11 * b) // 8
    assert a >= 0 and 8 * a + 11 * b == delta, delta
    tex = {"type": "diffuse", "texture": {"type": "checkerboard", "color0": (0.2, 0.3, 0.4), "color1": (0.8, 0.7, 0.6), "scale": (3, 3)}}
    return ([hm.MeshSpec(f"pad{i}", [], hm.WHITE) for i in range(a)] +
            [hm.MeshSpec(f"padtex{i}", [], hm.WHITE, bsdf=tex) for i in range(b)])


def padded_to(hm, meshes, key, target):
    return meshes + faceless_pads(hm, target - table_plan(hm.flatten(meshes, W, H))[key])


LONG_CDF_ZERO_FACES = (0, 1, 4002, 4003, 4004, 8005, 8006)
# radii of the long-CDF blob: at the first the fp32 CDF's last entry, sum * (1 / sum), rounds to 1, at the second to 1 - 2^-24
LONG_CDF_RADIUS = {False: 80.25, True: 80.0}


def long_cdf_blob(hm, radius):
    """an emissive blob of 8000 triangles and 7 of zero area (two first, three in the middle, two last): an area emitter
    whose CDF has 8008 entries and is exactly flat at the zero-area faces"""
    blob = hm.blob_mesh("long_cdf", (278, 330, 200), radius, 41, 100, hm.WHITE, seed=3)
    f = list(blob.faces)
    assert len(f) == 2 * 100 * 40
    deg = lambda p: (p, p, p)
    mid = len(f) // 2
    blob.faces = [deg(f[0][0]), deg(f[0][1])] + f[:mid] + [deg(f[mid][0])] * 3 + f[mid:] + [deg(f[-1][2]), deg(f[-1][1])]
    blob.radiance = (2.0, 1.5, 1.0)
    return blob


def blob(hm, n_theta, n_phi, conductor=False):
    """2 n_phi (n_theta - 1) triangles above the boxes"""
    b = hm.blob_mesh("blob", (278, 420, 150), 50, n_theta, n_phi, hm.WHITE, seed=5)
    if conductor:
        b.bsdf = {"type": "roughconductor", "alpha": 0.2, "eta": (0.2, 0.92, 1.1), "k": (3.9, 2.45, 2.14), "twosided": True}
    return b


def material_wall(hm, n):
    """n small squares in front of the back wall, each with a BSDF of its own, cycling through every kind the back end takes"""
    cu = dict(type="roughconductor", eta=(0.2, 0.92, 1.1), k=(3.9, 2.45, 2.14))
    kinds = [None,                                                                           # diffuse rgb
             {"type": "diffuse", "texture": {"type": "checkerboard", "color0": (0.9, 0.2, 0.1), "color1": (0.1, 0.3, 0.8),
                                             "scale": (4, 4)}},
             "uniform", "regular",
             dict(cu, alpha=0.2),                                                            # one-sided, sample_visible off
             dict(cu, alpha=(0.1, 0.3), sample_visible=True, twosided=True),
             dict(type="roughdielectric", alpha=0.15, int_ior=1.5, ext_ior=1.0),
             dict(cu, alpha=0.35, sample_visible=True),                                      # one-sided, sample_visible on
             dict(cu, alpha=0.05, twosided=True),                                            # two-sided, sample_visible off
             dict(type="roughdielectric", alpha=0.3, int_ior=1.33, ext_ior=1.0, sample_visible=True),
             {"type": "diffuse", "twosided": True}]
    rows = (n + 19) // 20
    out = []
    for i in range(n):
        cx, cy = 40 + (i % 20) * 25.0, 40 + (i // 20) * (470.0 / max(1, rows - 1))
        z, h = 440.0 + (i % 3) * 25.0, 10.0
        face = ((cx + h, cy - h, z), (cx - h, cy - h, z), (cx - h, cy + h, z), (cx + h, cy + h, z))
        refl = (0.2 + 0.6 * ((i * 7) % 11) / 10, 0.3 + 0.5 * ((i * 3) % 7) / 6, 0.25 + 0.5 * (i % 5) / 4)
        m = hm.MeshSpec(f"mat{i}", [face], refl, texcoords=[((0, 0), (1, 0), (1, 1), (0, 1))])
        kind = kinds[i % len(kinds)]
        if kind == "uniform":
            m.reflectance = 0.2 + 0.6 * (i % 9) / 8
        elif kind == "regular":
            m.reflectance = hm.Regular(400.0, 700.0, 0.1 + 0.8 * np.abs(np.sin(np.arange(6 + i % 5) * 0.7 + i)))
        else:
            m.bsdf = kind
        out.append(m)
    return out


# ----------------------------------------------------------------------------- the scene family
def _cbox(hm):
    return hm.cbox_meshes(), {}


def _small_staged(hm):          # 23 lamps (small_f4 988) and a glossy 192-triangle blob: 270 triangles, table_f4 2608
    return hm.cbox_meshes() + ceiling_quads(hm, 23, 12, (8, 8, 8), "lamp") + [blob(hm, 13, 8, conductor=True)], {}


def _nothing_staged(hm):        # 30 lamps (small_f4 1238) and a diffuse 144-triangle blob: table_f4 2654
    return hm.cbox_meshes() + ceiling_quads(hm, 30, 12, (8, 8, 8), "lamp") + [blob(hm, 10, 8)], {}


def _long_cdf(below_one):
    return lambda hm: (hm.cbox_meshes() + [long_cdf_blob(hm, LONG_CDF_RADIUS[below_one])], {})


def _many_emitters(n_quads, env_first):
    def make(hm):
        lamps = ceiling_quads(hm, n_quads - 1, 3, (20, 20, 20), "tiny")
        lamps.insert(n_quads // 2, zero_area_emitter(hm))
        return hm.cbox_meshes() + lamps, {"env": {"radiance": (0.05, 0.06, 0.08), "first": env_first}}
    return make


def _many_materials(hm):
    return hm.cbox_meshes() + material_wall(hm, 310), {}


def _small_boundary(target):    # 20 lamps and a diffuse 192-triangle blob (small_f4 882, table_f4 2466) padded to `target`
    def make(hm):
        return padded_to(hm, hm.cbox_meshes() + ceiling_quads(hm, 20, 12, (8, 8, 8), "lamp") + [blob(hm, 13, 8)], "small_f4", target), {}
    return make


def _table_boundary(target):    # 10 lamps and a glossy 256-triangle blob (small_f4 528, table_f4 2376) padded to `target`
    def make(hm):
        base = hm.cbox_meshes() + ceiling_quads(hm, 10, 12, (8, 8, 8), "lamp") + [blob(hm, 17, 8, conductor=True)]
        return padded_to(hm, base, "table_f4", target), {}
    return make


# name -> (MSK_LDS_SCENE_KB, tree in LDS, lds_tables, small tables in LDS, builder)
SCENES = {
    "cbox": (None, True, True, True, _cbox),
    "lds_tree__hbm_tables__small_staged": ("60", True, False, True, _small_staged),
    "lds_tree__nothing_staged": ("60", True, False, False, _nothing_staged),
    "hbm_tree__lds_tables": ("0", False, True, True, _cbox),
    "hbm_tree__small_staged": ("0", False, False, True, _small_staged),
    "hbm_tree__nothing_staged__long_cdf": ("0", False, False, False, _long_cdf(False)),
    "hbm_tree__nothing_staged__long_cdf_below_one": ("0", False, False, False, _long_cdf(True)),
    "many_emitters__997_env_first": ("0", False, False, False, _many_emitters(997, True)),
    "many_emitters__1000_env_last": ("0", False, False, False, _many_emitters(1000, False)),
    "many_materials": ("0", False, False, False, _many_materials),
    "small_f4_1024": ("0", False, False, True, _small_boundary(1024)),
    "small_f4_1025": ("0", False, False, False, _small_boundary(1025)),
    "table_f4_2560": ("0", False, True, True, _table_boundary(2560)),
    "table_f4_2561": ("0", False, False, True, _table_boundary(2561)),
}
BOUNDARY = {"small_f4_1024": ("small_f4", 1024), "small_f4_1025": ("small_f4", 1025),
            "table_f4_2560": ("table_f4", 2560), "table_f4_2561": ("table_f4", 2561)}
EXTRAS = ["hbm_tree__nothing_staged__long_cdf", "hbm_tree__nothing_staged__long_cdf_below_one", "many_emitters__997_env_first",
          "many_emitters__1000_env_last", "many_materials"]


@functools.lru_cache(maxsize=None)
def _flat(hm, name):
    meshes, kw = SCENES[name][4](hm)
    return hm.flatten(meshes, W, H, **kw)


def fused_expected(name):
    """MSK_FUSED=1 runs k_wavefront when tree and tables are both in LDS and k_wavefront_h when both are in HBM (msk_plan.h:
    fused_ok).  Its LDS sum fits every scene here: at most 36 KB of shading and 20 KB of traversal LDS for a tree in HBM."""
    _, tree_lds, lds_tables = SCENES[name][:3]
    return tree_lds == lds_tables


# The zero-area lamp next to an environment gives NaN samples, in the reference as in the oracle: after a BSDF sample that
# escapes to the environment, path.cpp:103-107 evaluates pdf_emitter_direct on the `ds` of that bounce's emitter sample
# (set_query runs for surface hits only), and when that sample went to the zero-area lamp its position, distance and normal
# are NaN (mesh.cpp:103-133 over a NaN CDF).  ImageBlock::put warns and splats them all the same (imageblock.cpp:57-81).
NAN_SCENES = {"many_emitters__997_env_first", "many_emitters__1000_env_last"}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(a, b):
    """bit for bit where finite, and non-finite in the same places (a NaN's sign and payload are the hardware's own)"""
    fin = np.isfinite(b)
    return a.shape == b.shape and np.array_equal(np.isfinite(a), fin) and np.array_equal(bits(a[fin]), bits(b[fin]))


# ----------------------------------------------------------------------------- CPU: the plan and the oracle
def test_cbox_table_counts(hostmirror):
    """8 mesh records + 8 BSDF records (56) + 1 emitter (3 + 24 of D65) + a 3-entry CDF (1) + CIE (72) = 164 small float4;
    and 32 triangles x 6 = 356 float4 of tables"""
    p = table_plan(_flat(hostmirror, "cbox"))
    assert (p["small_f4"], p["table_f4"]) == (164, 356)


@pytest.mark.parametrize("name", list(SCENES))
def test_scene_lands_on_its_side(hostmirror, abi, name):
    _, _, lds_tables, staged, _ = SCENES[name]
    flat = _flat(hostmirror, name)
    p = table_plan(flat)
    assert (p["lds_tables"], p["lds_tables"] or p["small_staged"]) == (lds_tables, staged), p
    if name in BOUNDARY:
        key, want = BOUNDARY[name]
        assert p[key] == want, p
        if key == "table_f4":
            assert p["small_staged"]             # the pair differs in lds_tables alone
        else:
            assert not p["lds_tables"]
    d = flat.desc
    if name.startswith("many_emitters"):
        n = int(name.split("__")[1].split("_")[0])
        assert d.n_emitters == n + 2             # the quads (one of zero area), the luminaire, the environment
        env = 0 if "env_first" in name else d.n_emitters - 1
        assert d.emitters[env].type == abi.MSK_EMITTER_CONSTANT
        assert all(d.emitters[i].type == abi.MSK_EMITTER_AREA for i in range(d.n_emitters) if i != env)
    if name == "many_materials":
        b = [d.bsdfs[i] for i in range(d.n_bsdfs)]
        assert d.n_bsdfs >= 300 and len({d.meshes[i].bsdf_id for i in range(d.n_meshes)}) == d.n_meshes
        assert max(x.back_bsdf for x in b) > 255
        for t in (abi.MSK_BSDF_DIFFUSE, abi.MSK_BSDF_ROUGHCONDUCTOR, abi.MSK_BSDF_ROUGHDIELECTRIC):
            assert max(i for i, x in enumerate(b) if x.type == t) > 255
        assert {(x.sample_visible, x.back_bsdf >= 0) for x in b if x.type == abi.MSK_BSDF_ROUGHCONDUCTOR} == {(0, 0), (0, 1), (1, 0), (1, 1)}
        assert d.n_textures > 0 and d.n_regular_spectra > 0 and any(x.reflectance_scale != 1 for x in b)


def _float64_cdf(flat, mesh):
    m = flat.desc.meshes[mesh]
    f = flat.faces[m.first_face:m.first_face + m.face_count].astype(np.int64) + m.first_vertex
    p = flat.vertices[:, :3].astype(np.float64)[f]                   # the fp32 positions, exactly
    a64 = 0.5 * np.linalg.norm(np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), axis=1)
    run = np.concatenate([[0.0], np.cumsum(a64)])
    return a64, run / run[-1], run[-1]


@pytest.mark.parametrize("below_one", [False, True], ids=["ends_at_1", "ends_below_1"])
def test_long_cdf_against_float64(hostmirror, oracle, below_one):
    """The area CDF of the 8007-face emitter (mesh.cpp:39-48, core/distribution.h:88-96: an fp32 running sum from 0,
    multiplied by 1.f / sum) against a float64 prefix sum over the same fp32 vertices."""
    flat = _flat(hostmirror, "hbm_tree__nothing_staged__long_cdf" + ("_below_one" if below_one else ""))
    mesh = flat.desc.n_meshes - 1
    o = oracle.scene(flat)
    try:
        area, cdf = o.mesh_tables(mesh)
    finally:
        o.close()
    a64, cdf64, total64 = _float64_cdf(flat, mesh)
    n = len(a64)
    assert n == 8007 and len(cdf) == n + 1
    assert tuple(np.nonzero(a64 == 0)[0]) == LONG_CDF_ZERO_FACES
    assert cdf[0] == 0 and (np.diff(cdf) >= 0).all()
    assert all(cdf[f + 1] == cdf[f] for f in LONG_CDF_ZERO_FACES)      # flat exactly where a face has no area
    # Recursive fp32 summation of n non-negative terms is off by at most (n - 1) u times their sum (u = eps32 / 2); each face
    # area carries a few u of itself (differences, cross product, dot, sqrt, x 0.5) and the normalisation two roundings.
    # Every normalised entry is therefore within (n / 2 + 4) eps32 of the float64 one, and k = 1 bounds that.
    eps32 = float(np.finfo(np.float32).eps)
    err = float(np.abs(cdf.astype(np.float64) - cdf64).max())
    assert err <= 1.0 * n * eps32, err
    assert abs(area - total64) <= 1.0 * n * eps32 * total64, (area, total64)          # the same sum, not normalised
    # The last entry is fp32 sum * (1 / sum), and that is not always 1.
    a32 = np.float32(area)
    assert cdf[-1] == a32 * (np.float32(1.0) / a32)
    # Below 1, a u in [cdf[n], 1) is clamped to the last face and reused above 1 (distribution.h:106-116).
    assert cdf[-1] == (np.float32(1.0) - np.float32(2.0 ** -24) if below_one else np.float32(1.0))


@pytest.mark.parametrize("name", list(SCENES))
def test_oracle_tree_equals_brute_force(hostmirror, abi, oracle, name):
    """The oracle's own BVH against its every-triangle loop (set_bvh(0)) on every scene of the family; finite weights."""
    o = oracle.scene(_flat(hostmirror, name))
    try:
        prm = abi.render_params(spp=2, seed=SEED)
        t0 = time.time()
        tree, st = o.render(prm, threads=8)
        o.set_bvh(0)
        brute, bst = o.render(prm, threads=8)
        print(f"\n[timing] {name}: oracle tree + brute force {time.time() - t0:.1f} s")
    finally:
        o.close()
    assert st.samples == bst.samples == W * H * 2 and st.invalid_samples == bst.invalid_samples
    assert np.array_equal(bits(tree), bits(brute))
    assert np.isfinite(tree[..., 3:]).all() and (tree[..., 4] > 0).all() and np.nanmax(tree[..., :3]) > 0
    if name in NAN_SCENES:
        assert st.invalid_samples > 0 and not np.isfinite(tree[..., :3]).all()
    else:
        assert st.invalid_samples == 0 and np.isfinite(tree).all()


# ----------------------------------------------------------------------------- GPU parity
_REF = {}


def oracle_film(hm, oracle, name, prm):
    """the oracle's film of the default parameters, once per scene"""
    if name not in _REF:
        o = oracle.scene(_flat(hm, name))
        try:
            t0 = time.time()
            _REF[name] = o.render(prm, threads=ORACLE_THREADS)
            print(f"\n[timing] {name}: oracle film {time.time() - t0:.1f} s")
        finally:
            o.close()
    return _REF[name]


def gpu_scene(abi, gpu_ctx, hm, monkeypatch, name):
    kb = SCENES[name][0]
    if kb is None:
        monkeypatch.delenv("MSK_LDS_SCENE_KB", raising=False)
    else:
        monkeypatch.setenv("MSK_LDS_SCENE_KB", kb)                 # read by msk_gpu_scene_create
    return abi.Scene(gpu_ctx, _flat(hm, name))


def launches(st):
    return f"trace {st.launches_trace} shade {st.launches_shade} wavefront {st.launches_wavefront}"


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SCENES))
def test_film_bit_exact_and_fused_probe(gpu_ctx, abi, hostmirror, oracle, monkeypatch, name):
    """The film (counter RNG, default settings), the same with MSK_SORT=0 and with MSK_FUSED=1, against the oracle bit for
    bit.  MSK_FUSED=1 also probes the placement: the whole pass runs in k_wavefront(_h) exactly when the plan allows it."""
    for k in ("MSK_FUSED", "MSK_SORT", "MSK_FUSED_HBM", "MSK_FUSED_TAIL_PCT", "MSK_BVH_BUILD", "MSK_WIDE_BVH", "MSK_QUANT_BVH"):
        monkeypatch.delenv(k, raising=False)
    prm = abi.render_params(spp=SPP, seed=SEED)
    ref, rst = oracle_film(hostmirror, oracle, name, prm)
    g = gpu_scene(abi, gpu_ctx, hostmirror, monkeypatch, name)
    try:
        t0 = time.time()
        film, st = g.render(prm)
        assert (st.samples, st.invalid_samples) == (rst.samples, rst.invalid_samples)
        assert same(film, ref), (int((bits(film) != bits(ref)).sum()), float(np.nanmax(np.abs(film - ref))))
        assert st.launches_shade > 0
        monkeypatch.setenv("MSK_SORT", "0")
        nosort, st0 = g.render(prm)
        monkeypatch.delenv("MSK_SORT")
        assert st0.samples == st.samples and same(nosort, film)
        monkeypatch.setenv("MSK_FUSED", "1")
        fused, stf = g.render(prm)
        monkeypatch.delenv("MSK_FUSED")
        assert (stf.samples, stf.invalid_samples) == (rst.samples, rst.invalid_samples)
        assert same(fused, ref)
        if fused_expected(name):
            assert stf.launches_wavefront > 0 and stf.launches_shade == 0 and stf.launches_trace == 0, launches(stf)
        else:
            assert stf.launches_wavefront == 0 and stf.launches_shade == stf.launches_trace > 0, launches(stf)
        p = table_plan(g.flat)
        print(f"\n[placement] {name}: table_f4 {p['table_f4']} small_f4 {p['small_f4']} tree {'LDS' if SCENES[name][1] else 'HBM'}; "
              f"default: {launches(st)}; MSK_FUSED=1: {launches(stf)}")
        print(f"[timing] {name}: three GPU renders {time.time() - t0:.1f} s")
    finally:
        g.close()


def pick_pixels(hm, abi, oracle, name, n=40):
    """n film pixels: up to 12 whose camera ray hits an emitter, up to 12 on a rough conductor or dielectric, the rest
    spread over the film.  -> (pixels, how many see an emitter, how many a glossy surface)"""
    flat = _flat(hm, name)
    d = flat.desc
    o = oracle.scene(flat)
    try:
        ys, xs = np.mgrid[0:H, 0:W]
        xs, ys = xs.ravel(), ys.ravel()
        hit = o.trace_closest(np.stack([o.camera_ray(0.5, x + 0.5, y + 0.5)[0] for x, y in zip(xs, ys)]))
    finally:
        o.close()
    mesh_of = np.repeat(np.arange(d.n_meshes), [d.meshes[i].face_count for i in range(d.n_meshes)])
    valid = np.isfinite(hit[:, 0])
    mesh = np.where(valid, mesh_of[np.where(valid, hit[:, 3].view(np.uint32), 0)], -1)
    emissive = np.array([m >= 0 and d.meshes[m].emitter_id >= 0 for m in mesh])
    glossy = np.array([m >= 0 and d.bsdfs[d.meshes[m].bsdf_id].type != abi.MSK_BSDF_DIFFUSE for m in mesh])
    pick = []
    for sel in (np.nonzero(emissive)[0], np.nonzero(glossy)[0]):
        if len(sel):
            pick += sel[np.linspace(0, len(sel) - 1, min(12, len(sel))).astype(int)].tolist()
    pick += [int(i) for i in np.random.RandomState(7).permutation(W * H) if i not in pick][:n - len(pick)]
    return np.stack([xs[pick], ys[pick]], 1).astype(np.int32), int(emissive[pick].sum()), int(glossy[pick].sum())


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SCENES))
def test_sample_pixels_bit_exact(gpu_ctx, abi, hostmirror, oracle, monkeypatch, name):
    pixels, n_em, n_gl = pick_pixels(hostmirror, abi, oracle, name)
    d = _flat(hostmirror, name).desc
    assert len(pixels) >= 32 and n_em > 0
    assert n_gl > 0 or all(d.bsdfs[i].type == abi.MSK_BSDF_DIFFUSE for i in range(d.n_bsdfs))
    prm = abi.render_params(spp=8, seed=SEED + 1)
    o = oracle.scene(_flat(hostmirror, name))
    g = gpu_scene(abi, gpu_ctx, hostmirror, monkeypatch, name)
    try:
        t0 = time.time()
        gx, gp = g.sample_pixels(prm, pixels)
        ox, op = o.sample_pixels(prm, pixels)
        assert np.array_equal(bits(gp), bits(op))
        bad = [i for i in range(len(pixels)) if not same(gx[i], ox[i])]
        assert not bad, pixels[bad[:6]].tolist()
        assert np.nanmax(gx) > 0
        print(f"\n[timing] {name}: sample_pixels {len(pixels)} px ({n_em} on emitters, {n_gl} glossy) {time.time() - t0:.1f} s")
    finally:
        g.close()
        o.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", EXTRAS)
def test_serial_aov_and_shard_bit_exact(gpu_ctx, abi, hostmirror, oracle, monkeypatch, name):
    """The scenes with many emitters, many materials and the long CDF through the other entry points: the per-block PCG32
    film (k_path_serial), the "aov" integrator with depth, shading normal and nested path channels (the general shading
    variant, no fused tail), one tile shard; many_materials also with the tree built on the device (MSK_BVH_BUILD=gpu: the
    material class bits written by k_tris)."""
    for k in ("MSK_FUSED", "MSK_SORT", "MSK_BVH_BUILD"):
        monkeypatch.delenv(k, raising=False)
    o = oracle.scene(_flat(hostmirror, name))
    t0 = time.time()
    try:
        g = gpu_scene(abi, gpu_ctx, hostmirror, monkeypatch, name)
        try:
            pcg = abi.render_params(spp=SPP, seed=SEED, rng_mode=abi.MSK_RNG_PCG_BLOCK)
            film, st = g.render(pcg)
            ref, rst = o.render(pcg, threads=ORACLE_THREADS)
            assert (st.samples, st.invalid_samples) == (rst.samples, rst.invalid_samples)
            assert same(film, ref), "PCG block"

            types = [abi.MSK_AOV_DEPTH, abi.MSK_AOV_SH_NORMAL, abi.MSK_AOV_PATH_RGBA]
            prm = abi.render_params(spp=SPP, seed=SEED + 2)
            film, st = g.render_aov(prm, types)
            ref, rst = o.render_aov(prm, types, threads=ORACLE_THREADS)
            assert st.launches_wavefront == 0 and (st.samples, st.invalid_samples) == (rst.samples, rst.invalid_samples)
            assert film.shape == ref.shape == (H, W, 5 + 1 + 3 + 4)
            assert same(film, ref), "aov"

            shard = abi.render_params(spp=SPP, seed=SEED, block_first=1, block_stride=2)
            film, st = g.render(shard)
            ref, rst = o.render(shard, threads=ORACLE_THREADS)
            assert (st.samples, st.invalid_samples) == (rst.samples, rst.invalid_samples) and 0 < st.samples < W * H * SPP
            assert same(film, ref), "tile shard"
        finally:
            g.close()
        if name == "many_materials":
            monkeypatch.setenv("MSK_BVH_BUILD", "gpu")
            g = gpu_scene(abi, gpu_ctx, hostmirror, monkeypatch, name)
            try:
                prm = abi.render_params(spp=SPP, seed=SEED)
                film, st = g.render(prm)
                ref, rst = oracle_film(hostmirror, oracle, name, prm)
                assert (st.samples, st.invalid_samples) == (rst.samples, rst.invalid_samples)
                assert same(film, ref), "MSK_BVH_BUILD=gpu"
            finally:
                g.close()
        print(f"\n[timing] {name}: PCG block + aov + tile shard{' + device-built tree' if name == 'many_materials' else ''}, "
              f"with the oracle, {time.time() - t0:.1f} s")
    finally:
        o.close()
