"""Scene creation's host side on a CPU: csrc/msk_scene_tables.h (every refusal of a descriptor, every packed table) and the
placement of csrc/msk_plan.h (SceneKnobs, place_tables, place_tree), as printed by tests/native/scene_tables_check.cpp.

THE REFERENCE is msk_gpu_scene_create_ext of csrc/msk_gpu.hip at commit e7567ac, the function these headers were cut from:
  lines 252-585     the 67 refusals: REFUSALS below holds each one's code and the distinguishing words of its format string,
                    copied from there, in the order the function made them
  lines 710-793     the placement ladder: parent_tree / parent_sizes below transcribe it statement by statement, never from msk_plan.h
The table sizes are also held against table_plan() of tests/test_table_placement.py.  (That the packed BYTES are the parent's is
not a test: EXPERIMENTS.md records the digests of this check's `tables` mode next to those of the parent's code on the same
descriptors.)"""
import itertools
import os
import re
import subprocess
import types

import pytest

import test_table_placement

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = -1, -5          # include/msk_gpu.h: MSK_ERR_INVALID_ARG, MSK_ERR_UNSUPPORTED

# (case of scene_tables_check refusals, code, words of the parent's format string)
REFUSALS = [
    ("abi_version", INVALID, "msk_gpu_scene_create: abi_version 7 != 8"),
    ("film", INVALID, "msk_gpu_scene_create: invalid film 16x8 radius 0"),
    ("crop", INVALID, "Invalid crop window specification! offset (9, 0) + crop size (8, 8) vs full size (16, 8)"),
    ("spectral_tables", INVALID, "msk_gpu_scene_create: spectral tables missing"),
    ("geometry_arrays", INVALID, "msk_gpu_scene_create: geometry arrays missing"),
    ("bsdf_emitter_arrays", INVALID, "msk_gpu_scene_create: bsdf / emitter arrays missing"),
    ("too_many_triangles", UNSUPPORTED, "triangles, this back end addresses fewer than 2^26"),
    ("mesh_range", INVALID, "mesh 1: vertex/face range exceeds the arrays"),
    ("mesh_bsdf_id", INVALID, "mesh 0: bsdf_id 2 out of range"),
    ("mesh_emitter_id", INVALID, "mesh 0: emitter_id 1 out of range"),
    ("mesh_emitter_back", INVALID, "mesh 0: emitter 0 does not point back at it"),
    ("face_in_two_meshes", INVALID, "face 1 belongs to two meshes"),
    ("vertex_index", INVALID, "mesh 0 face 1: vertex index 4 out of range"),
    ("vertex_not_finite", INVALID, "mesh 1 vertex 1: non-finite position"),
    ("face_in_no_mesh", INVALID, "face 2 belongs to no mesh"),
    ("regular_arrays", INVALID, "msk_gpu_scene_create: regular spectrum arrays missing"),
    ("regular_too_many_values", UNSUPPORTED, "tabulated spectrum values, a spectrum record addresses fewer than 2^24"),
    ("regular_one_entry", INVALID, "regular spectrum 1: ContinuousDistribution: needs at least two entries!"),
    ("regular_too_long", UNSUPPORTED, "regular spectrum 1: 96 values, this back end takes at most 95"),
    ("regular_range", INVALID, "regular spectrum 0: ContinuousDistribution: invalid range!"),
    ("regular_values_exceed", INVALID, "regular spectrum 1: values [6, 9) exceed the 8 in regular_values"),
    ("regular_negative", INVALID, "regular spectrum 0: ContinuousDistribution: entries must be non-negative!"),
    ("regular_no_mass", INVALID, "regular spectrum 1: ContinuousDistribution: no probability mass found!"),
    ("spectrum_names_regular", INVALID, "bsdf 1: eta names regular spectrum 3 of 2"),
    ("spectrum_scale", INVALID, "bsdf 1: the scale of k must not be negative"),
    ("texture_array", INVALID, "msk_gpu_scene_create: texture array missing"),
    ("texture_type", UNSUPPORTED, "texture 0: type 7 is not supported by this back end (checkerboard, bitmap)"),
    ("bitmap_size", INVALID, "texture 0: a bitmap of 2 x 0 texels (width and height must be at least 1)"),
    ("bitmap_past_pool", INVALID, "texture 0: texels 1 + 2 x 2 reach past the scene's n_texels 4"),
    ("bitmap_pool_missing", INVALID, "texture 0: a bitmap, but the scene's texels array is missing"),
    ("bitmap_nan", INVALID, "texture 0: texel 2 holds a NaN coefficient"),
    ("bsdf_type", UNSUPPORTED, "bsdf 1: type 5 is not supported by this back end (diffuse, roughconductor, roughdielectric, dielectric, conductor)"),
    ("bsdf_back", INVALID, "bsdf 1: back_bsdf 2 out of range"),
    ("bsdf_roughness", INVALID, "bsdf 1: negative roughness"),
    ("bsdf_ior", INVALID, "bsdf 1: the relative index of refraction must be positive"),
    ("dielectric_nested", INVALID, "bsdf 1: Only materials without a transmission component can be nested!"),
    ("conductor_with_ior", INVALID, "bsdf 1: type 4 is not supported for a descriptor with a relative index of refraction (ior_eta 1.5, ior_inv_eta 0.666667): "
                                    "a conductor has none (1 / 1, or 0 / 0 = unset); its eta and k are spectra"),
    ("bsdf_texture_range", INVALID, "bsdf 0: reflectance_texture 2 out of range"),
    ("bsdf_reflectance_scale", INVALID, "bsdf 1: reflectance_scale must be finite and non-negative (1 for an srgb reflectance)"),
    ("bsdf_textured_not_diffuse", UNSUPPORTED, "bsdf 0: only the diffuse reflectance can be textured"),
    ("bsdf_regular_and_texture", INVALID, "bsdf 0: reflectance_regular names the reflectance of an untextured diffuse BSDF"),
    ("envmap_without_image", INVALID, "emitter 1: an envmap emitter needs its image (msk_gpu_scene_create_env with an msk_envmap_desc)"),
    ("envmap_regular_radiance", INVALID, "emitter 1: an envmap emitter has no tabulated radiance (radiance_regular must be 0)"),
    ("envmap_scale", INVALID, "emitter 1: envmap: the scale must be finite and non-negative"),
    ("two_environments", INVALID, "Can only have one environment light"),
    ("environment_with_mesh", INVALID, "emitter 0: an environment emitter has no mesh (mesh_id must be -1)"),
    ("area_mesh_back", INVALID, "emitter 1: mesh_id 0 does not point back at it"),
    ("area_mesh_without_faces", INVALID, "emitter 1: its mesh has no faces"),
    ("point_with_mesh", INVALID, "emitter 1: a point emitter has no mesh (mesh_id must be -1)"),
    ("point_two_positions", INVALID, "emitter 1: a point emitter with two positions (msk_point_desc 1 is its second)"),
    ("point_without_position", INVALID, "emitter 1: a point emitter needs its position (msk_gpu_scene_create_ext with an msk_point_desc)"),
    ("point_not_finite", INVALID, "emitter 1: a point emitter's position must be finite"),
    ("emitter_type", UNSUPPORTED, "emitter 1: type 9 is not supported (area, constant, envmap, point)"),
    ("emitter_names_regular", INVALID, "emitter 0: radiance names regular spectrum 3 of 2"),
    ("points_missing", INVALID, "msk_scene_ext: n_points 1 without points"),
    ("point_desc_range", INVALID, "msk_point_desc 1: emitter 9 out of range (the scene has 2)"),
    ("point_desc_not_a_point", INVALID, "msk_point_desc 1: emitter 0 is of type 0, not a point emitter (type 3)"),
    ("image_without_envmap", INVALID, "envmap: an image was given, but the scene has no envmap emitter (type 2)"),
    ("envmap_size", INVALID, "envmap: an image of 0 x 2 texels (width and height must be at least 1)"),
    ("envmap_too_large", UNSUPPORTED, "envmap: 16384 x 16384 texels, this back end takes fewer than 2^28"),
    ("envmap_arrays", INVALID, "envmap: texels / weights array missing"),
    ("envmap_factor", INVALID, "envmap: texel 2: the factor w must be finite and non-negative"),
    ("envmap_nan", INVALID, "envmap: texel 5 holds a NaN coefficient"),
    ("envmap_weights", INVALID, "envmap: weights must be finite and non-negative"),          # msk_envmap.h's text, handed on as "%s"
    ("envmap_rotation", INVALID, "envmap: to_world must be a rotation"),
    ("envmap_pool_offsets", UNSUPPORTED, "envmap: 4 x 2 texels do not fit the texel pool's 32-bit offsets"),
    ("pad_scale", INVALID, "MSK_PAD_SCALE=\"1e-9\": the padding of the boxes must be a number in [1e-7, 1e-3] of the scene's scale "
                           "(default 1e-5; the slab arithmetic needs a few 1e-7)"),
]
N_PARENT_REFUSALS = 67                 # `return fail(ctx, ...)` in lines 252-585 of the parent's msk_gpu.hip
# the same refusal a second way, and descriptors with two faults: (case, the case whose message it must carry)
SAME_AS = [("pad_scale_garbage", "pad_scale")]
TWO_FAULTS = [("two_abi_then_film", "abi_version"), ("two_mesh_then_bsdf", "mesh_bsdf_id"), ("two_regular_then_texture", "regular_one_entry"),
              ("two_texture_then_bsdf", "texture_type"), ("two_bsdf_then_emitter", "bsdf_back"), ("two_emitter_then_image", None),
              ("two_image_then_pad_scale", "envmap_rotation"), ("two_first_bsdf_then_second", None)]
TWO_FAULTS_TEXT = {"two_emitter_then_image": "emitter 0: radiance names regular spectrum 3 of 0",
                   "two_first_bsdf_then_second": "bsdf 0: reflectance_scale must be finite and non-negative (1 for an srgb reflectance)"}

SCENES = ["quad", "bitmap", "checkerboard", "regular", "envmap", "point_conductor", "constant_sky", "zero_faces"]
VECTORS = ["pos", "tv", "tn", "tuv", "mesh_info", "bsdfs", "emitters", "d65", "emitter_grid", "cdf_all", "spectra_pool", "cie", "texels",
           "bvh_nodes", "bvh_tris", "bvh_bounds"]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("scene_tables") / "scene_tables_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", out, os.path.join(ROOT, "tests", "native", "scene_tables_check.cpp")])
    return out


def run(exe, what, knobs=None):
    env = {k: v for k, v in os.environ.items() if not k.startswith("MSK_")}
    env.update(knobs or {})
    r = subprocess.run([exe, what], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    return r.stdout.splitlines()


# ----------------------------------------------------------------------------- refusals
def test_every_refusal_of_the_parent_keeps_its_code_and_words(exe):
    got = {}
    for line in run(exe, "refusals"):
        name, code, text = line.split(" ", 2)
        got[name] = (int(code), text)
    assert len(REFUSALS) == len({r[0] for r in REFUSALS}) == len({r[2] for r in REFUSALS}) == N_PARENT_REFUSALS
    header = open(os.path.join(ROOT, "misaki-render_amd", "csrc", "msk_scene_tables.h")).read()
    # A cross-check only, on the header's text as it is written today: the move added and lost no `return refuse(msg, ...)`.  What
    # holds each refusal to the parent is the per-case assertion below.
    assert len(re.findall(r"return refuse\(msg,", header)) == N_PARENT_REFUSALS
    assert set(got) == {r[0] for r in REFUSALS} | {c for c, _ in SAME_AS} | {c for c, _ in TWO_FAULTS}
    for name, code, words in REFUSALS:
        assert got[name][0] == code and words in got[name][1], (name, got[name])
    for name, first in SAME_AS:
        assert got[name][0] == got[first][0] and got[name][1] == got[first][1].replace("1e-9", "1e-5x"), (name, got[name])


def test_a_descriptor_with_two_faults_gets_the_earlier_message(exe):
    got = {}
    for line in run(exe, "refusals"):
        name, code, text = line.split(" ", 2)
        got[name] = (int(code), text)
    for name, first in TWO_FAULTS:
        assert got[name] == (got[first] if first else (INVALID, TWO_FAULTS_TEXT[name])), (name, got[name])


# ----------------------------------------------------------------------------- tables
def parse_tables(lines):
    scenes, cur = {}, None
    for l in lines:
        key, _, rest = l.partition(" ")
        if key == "scene":
            cur = scenes.setdefault(rest, {"vec": {}})
        elif key == "vec":
            name, n, digest = rest.split()
            cur["vec"][name] = (int(n), digest)
        elif key in ("flags", "counts", "floats"):
            cur.update((a, b) for a, b in (kv.split("=") for kv in rest.split()))
        else:
            cur[key] = rest.split()
    return scenes


# name -> (faces, meshes, bsdfs, emitters, textures, regular values, flags that are set)
EXPECT = {
    "quad": (4, 2, 2, 1, 0, 0, {"all_diffuse"}),
    "bitmap": (4, 2, 2, 1, 1, 0, {"has_bitmap", "any_normals", "any_uvs"}),
    "checkerboard": (4, 2, 2, 1, 1, 0, {"any_uvs"}),
    "regular": (4, 2, 2, 1, 0, 8, {"has_regular"}),
    "envmap": (4, 2, 2, 2, 0, 0, {"has_envmap"}),
    "point_conductor": (4, 2, 2, 2, 0, 0, {"has_delta"}),
    "constant_sky": (4, 2, 2, 2, 0, 0, set()),
    "zero_faces": (0, 1, 1, 0, 0, 0, {"all_diffuse"}),
}
FLAGS = ["all_diffuse", "has_regular", "has_dielectric", "has_bitmap", "has_envmap", "has_delta", "any_normals", "any_uvs"]


def test_tables_have_the_shape_the_descriptor_gives_them(exe):
    lines = run(exe, "tables")
    scenes = parse_tables(lines)
    assert list(scenes) == SCENES
    assert lines == run(exe, "tables")                                   # the digests are stable from run to run
    for name, (nf, nm, nb, ne, nt, nv, flags) in EXPECT.items():
        s, vec = scenes[name], scenes[name]["vec"]
        assert "refused" not in s and set(vec) == set(VECTORS), name
        assert {f for f in FLAGS if s[f] == "1"} == flags, name
        n_bsdf_f4 = 7 * nb + 3 * nt
        assert (int(s["n_bsdf_f4"]), int(s["n_textures"]), int(s["tex_base"])) == (n_bsdf_f4, nt, 7 * nb), name
        area = [e for e in s.get("emitter_meta", []) if int(e.split(",")[0]) < nm]
        cdf_len = sum(int(e.split(",")[2]) + 1 for e in area) or 1
        texels = {"bitmap": 4 * 4, "envmap": 4 * (3 + 8 + 1 + 3)}.get(name, 0)   # envmap: header 3 float4, 8 texels, marginal 3 -> 4 floats, rows 2 x 5 -> 12 floats
        want = dict(pos=9 * nf, tv=12 * nf, tn=12 * nf if "any_normals" in flags else 0, tuv=8 * nf if "any_uvs" in flags else 0, mesh_info=4 * max(1, nm),
                    bsdfs=4 * n_bsdf_f4, emitters=8 * max(1, ne), d65=95 * max(1, ne), emitter_grid=4 * max(1, ne), cdf_all=cdf_len, spectra_pool=max(1, nv),
                    cie=285, texels=texels, bvh_tris=16 * nf, bvh_bounds=8 * nf)
        assert {k: vec[k][0] for k in want} == want, name
        assert vec["bvh_nodes"][0] % 16 == 0
        # the integer words of the records
        assert [int(x) for x in s.get("tri_mesh", [])] == ([0, 0, 1, 1] if nf else [])
        if nf:
            em = 1 if name == "constant_sky" else 0
            normals_uvs = {"bitmap": 3, "checkerboard": 2}.get(name, 0)
            assert [int(x) for x in s["mesh_info"]] == [0, -1, normals_uvs, 0, 1, em, 0, 2], name
            assert s["cdf"] == ["0", "0.5", "1"], name                   # two triangles of one area: the CDF ends at 1
            assert s["emitter_meta"][em] == "1,2,2,0,93" if name != "regular" else s["emitter_meta"][em] == "1,2,2,0,1"
            conductor = name == "point_conductor"
            tex_off = 14 if nt else 0
            assert s["bsdf_words"] == [f"{4 if conductor else 0},{0 if conductor else -1},0,{tex_off}", "0,-1,0,0"], name
            # the material class of every triangle: 0 for the diffuse ones, and 4 & 3 = 0 for the conductor
            assert sorted(s["classes"]) == [f"{t}:0" for t in range(4)], name
        else:
            assert s["cdf"] == ["0"] and vec["bvh_nodes"][0] == 0
        assert s["types"] == [f"e{t}" for t in {"envmap": [0, 2], "point_conductor": [0, 3], "constant_sky": [1, 0]}.get(name, [0] * ne)] + \
            [f"b{4 if name == 'point_conductor' and b == 0 else 0}" for b in range(nb)], name
        env = {"envmap": 1, "constant_sky": 0}.get(name, -1)
        assert int(s["env_emitter"]) == env
        assert (float(s["env_radius"]) > 0) == (env >= 0)
        if env >= 0:                                                     # {0xffffffff, block offset, is image, 0}
            assert s["emitter_meta"][env].split(",")[:4] == ["4294967295", "0", "1" if name == "envmap" else "0", "0"]
        if name == "point_conductor":
            assert s["emitter_meta"][1].split(",")[0] == str(0xfffffffe)
        if name == "bitmap":
            assert s["texture_words"] == ["0,2,2,2"]                     # first texel, width, height, type
        # 0.5e-5 of the scene's scale: the unit cube's diagonal
        assert float(s["tri_pad"]) == pytest.approx(0.5e-5 * 3 ** 0.5 if nf else 0.5e-5, rel=1e-6)
    assert scenes["quad"]["vec"]["bvh_tris"] == scenes["constant_sky"]["vec"]["bvh_tris"]      # class 0 everywhere: tagging changes no bit


def test_pad_scale_is_read_from_the_environment_and_refused_in_its_place(exe):
    a = parse_tables(run(exe, "tables", {"MSK_PAD_SCALE": "1e-6"}))
    assert float(a["quad"]["tri_pad"]) == pytest.approx(0.5e-6 * 3 ** 0.5, rel=1e-6)
    b = parse_tables(run(exe, "tables", {"MSK_PAD_SCALE": "0"}))
    assert all(s["refused"][0] == str(INVALID) and s["refused"][1] == 'MSK_PAD_SCALE="0":' for s in b.values())


# ----------------------------------------------------------------------------- placement
MSK_BLOCK = 256                        # msk_layout.h
TREES = [(31, 32, 6), (199, 379, 9), (200, 379, 9), (3, 510, 11), (3, 510, 15), (40000, 70000, 24), (3000, 3001, 250)]
WIDES = [(1, 3, 5, 1, 1), (0, 0, 7, 1, 1), (1, 2, 12, 0, 1), (1, 9, 40, 0, 0)]
COUNTS = [(32, 8, 8, 0, 1, 3, 0), (396, 10, 10, 1, 1, 3, 4), (396, 10, 10, 1, 1, 3, 5), (4000, 90, 118, 2, 1, 3, 8), (4000, 90, 118, 2, 1, 3, 9),
          (0, 0, 0, 0, 0, 1, 0), (2000, 1000, 1, 0, 999, 2997, 0), (70000, 3, 3, 1, 2, 8008, 190)]
KNOB_SETS = [{}, {"MSK_LDS_SCENE_KB": "0"}, {"MSK_LDS_SCENE_KB": "60"}, {"MSK_LDS_SCENE_KB": ""}, {"MSK_WIDE_BVH": "8"}, {"MSK_WIDE_BVH": "0"},
             {"MSK_QUANT_BVH": "0"}, {"MSK_QUANT_BVH": "1"}, {"MSK_WIDE_LDS": "1"}, {"MSK_STACK_CAP": "8"}, {"MSK_STACK_CAP": "1"}, {"MSK_STACK_CAP": "42"},
             {"MSK_WIDE_BVH": "8", "MSK_STACK_CAP": "64"}, {"MSK_COLLAPSE_OPTIMAL": "0", "MSK_BVH_BUILD": "gpu"}]


def parent_tree(env, n_nodes, n_tris, max_depth, root_is_leaf, ok8, depth8, depth4, has_half, has_byte):
    """msk_gpu.hip at e7567ac, lines 679 and 710-784, statement by statement.  collapse8 / collapse4 are stood in for by what the
    case says they return; `asked` records which ran, in order."""
    def env_u32(name, default):                                   # msk_plan.h:32-35
        v = env.get(name)
        return int(v) if v else default
    asked = ""
    n_nodes4 = n_nodes // 2 + 1                                   # what the check's collapse4 reports
    stack_entries = (max_depth + 2 + 3) & ~3                                                                          # 679
    stack_bytes = stack_entries * MSK_BLOCK * 4                                                                       # 711
    scene_bytes = n_nodes * 64 + n_tris * 96                                                                          # 712
    lds_cap = int(env["MSK_LDS_SCENE_KB"] or 0) * 1024 if "MSK_LDS_SCENE_KB" in env else 48 * 1024                    # 713 (atoi("") = 0)
    lds_scene = scene_bytes <= lds_cap and stack_bytes + scene_bytes <= 64 * 1024                                     # 714
    trace_lds = stack_bytes + (scene_bytes if lds_scene else 0)                                                       # 715
    mode = 0 if lds_scene else 1                                                                                      # 716
    wide = env_u32("MSK_WIDE_BVH", 4)
    took8 = False
    if not lds_scene and wide == 8 and not root_is_leaf:                                                              # 719
        asked += "8"
        took8 = bool(ok8)
    if took8:
        stack_entries = (7 * depth8 + 2 + 3) & ~3                                                                     # 724
        mode = 4                                                                                                      # 725
    elif not lds_scene and wide and not root_is_leaf:                                                                 # 727
        asked += "4"                                                                                                  # 729
        stack_entries = (3 * depth4 + 2 + 3) & ~3                                                                     # 738
        mode = 2                                                                                                      # 739
        if env_u32("MSK_QUANT_BVH", 2) == 2 and has_half:                                                             # 745
            mode = 6                                                                                                  # 750
        elif env_u32("MSK_QUANT_BVH", 2) and has_byte:                                                                # 752
            mode = 5                                                                                                  # 756
    elif lds_scene and env_u32("MSK_WIDE_LDS", 0) and not root_is_leaf:                                               # 766
        asked += "4"                                                                                                  # 769
        stack_entries = (3 * depth4 + 2 + 3) & ~3                                                                     # 773
        trace_lds = stack_entries * MSK_BLOCK * 4 + (n_nodes4 * 128 + n_tris * 96)                                    # 774
        mode = 3                                                                                                      # 775
    stack_total = stack_entries                                                                                       # 777
    if mode in (1, 2, 4, 5, 6):                                                                                       # 778 (msk_plan.h: tree_in_hbm)
        stack_entries = min(stack_total, max(4, env_u32("MSK_STACK_CAP", 16) & ~3))                                   # 782
        trace_lds = stack_entries * MSK_BLOCK * 4 + MSK_BLOCK * 16                                                    # 783
    return (f"tree {n_nodes} {n_tris} {max_depth} {int(root_is_leaf)} {ok8} {depth8} {depth4} {has_half} {has_byte} | "
            f"{mode} {int(lds_scene)} {stack_entries} {stack_total} {trace_lds} {stack_bytes} {asked or '-'}")


def parent_sizes(n_faces, n_meshes, n_bsdfs, n_textures, n_emitters, cdf_len, n_spectra):
    """lines 382 and 786-793"""
    u32 = lambda x: x & 0xffffffff
    n_bsdf_f4 = u32(max(1, n_bsdfs) * 7 + n_textures * 3)                                                             # 382
    small_f4 = n_meshes + n_bsdf_f4 + u32(n_emitters * 3) + u32(n_emitters * 95 + 3) // 4 + u32(cdf_len + 3) // 4 + 72 + u32(n_spectra + 3) // 4
    table_bytes = (n_faces * 6 + small_f4) * 16                                                                       # 786-787
    lds_tables = table_bytes <= 40 * 1024                                                                             # 788
    small_bytes = small_f4 * 16                                                                                       # 791
    small_staged = small_bytes if small_bytes <= 16 * 1024 else 0                                                     # 792 (MSK_SMALL_TABLES_KB = 16)
    shade_lds = (table_bytes if lds_tables else small_staged) + (256 // 64) * (128 * 5 // 2) * 16                     # 793
    return table_bytes, small_bytes, lds_tables, shade_lds


def fake_flat(n_faces, n_meshes, n_bsdfs, n_textures, n_emitters, cdf_len, n_spectra):
    """a descriptor with these counts, as far as table_plan() of test_table_placement.py reads one: the CDF's entries belong to
    one area emitter on mesh 0, the other emitters have no mesh"""
    ns = types.SimpleNamespace
    emitters = [ns(mesh_id=0 if k == 0 and cdf_len > 1 else -1) for k in range(n_emitters)]
    meshes = [ns(face_count=cdf_len - 1 if k == 0 else 0) for k in range(max(1, n_meshes))]
    return ns(desc=ns(emitters=emitters, meshes=meshes, n_emitters=n_emitters, n_bsdfs=n_bsdfs, n_textures=n_textures, n_meshes=n_meshes,
                      n_faces=n_faces, n_regular_values=n_spectra))


@pytest.mark.parametrize("knobs", KNOB_SETS, ids=lambda k: ",".join(f"{a}={b}" for a, b in k.items()) or "defaults")
def test_placement_is_what_the_ladder_decided(exe, knobs):
    lines = run(exe, "placement", knobs)
    got = [l for l in lines if l.startswith("tree ")]
    want = [parent_tree(knobs, t[0], t[1], t[2], bool(leaf), *w) for t, leaf, w in itertools.product(TREES, (0, 1), WIDES)]
    assert len(got) == len(want) == len(TREES) * 2 * len(WIDES)
    for g, w in zip(got, want):
        assert g == w, f"{knobs}\nplacement: {g}\nparent:    {w}"
    sizes = [l for l in lines if l.startswith("sizes ")]
    assert len(sizes) == len(COUNTS)
    for l, c in zip(sizes, COUNTS):
        ins, outs = (tuple(int(x) for x in part.split()) for part in l[len("sizes "):].split("|"))
        assert ins == c
        table_bytes, small_bytes, lds_tables, shade_lds = parent_sizes(*c)
        assert outs == (table_bytes, small_bytes, int(lds_tables), outs[3], shade_lds), (c, outs)
        assert outs[3] == shade_lds - 20480                              # what a block stages: without the done-queues
        # ... and the mirror the GPU tests of the placement pin their scenes with
        p = test_table_placement.table_plan(fake_flat(*c))
        assert (p["table_f4"] * 16, p["small_f4"] * 16, p["lds_tables"]) == (table_bytes, small_bytes, lds_tables), (c, p)
        assert (p["lds_tables"] or p["small_staged"]) == (outs[3] > 0), (c, p)


def test_the_cases_reach_every_form_and_both_sides_of_every_limit(exe):
    rows = []
    for k in KNOB_SETS:
        rows += [(tuple(k.items()), l.split()) for l in run(exe, "placement", k) if l.startswith("tree ")]
    mode = lambda r: int(r[1][11])
    asked = lambda r: r[1][17]
    assert {mode(r) for r in rows} == set(range(7))
    assert {asked(r) for r in rows} == {"-", "4", "8", "84"}                                 # "84": collapse8 refused, the 4-wide form is walked
    default = [r[1] for r in rows if r[0] == ()]
    lds = {(int(r[1]), int(r[12])) for r in default if r[2] == "379"}
    assert lds == {(199, 1), (200, 0)}                                                       # 48 KB of tree met exactly, missed by one node
    assert {(int(r[3]), int(r[12])) for r in default if r[2] == "510"} == {(11, 1), (15, 0)}       # 64 KB with the stack met exactly, missed by 4 KB
    sizes = [l.split() for l in run(exe, "placement") if l.startswith("sizes ")]
    assert [(int(s[9]), int(s[11])) for s in sizes[1:3]] == [(40960, 1), (40976, 0)]         # lds_tables at 2560 float4 and not at 2561
    assert [(int(s[10]), int(s[12])) for s in sizes[3:5]] == [(16384, 16384), (16400, 0)]    # the small tables staged at 1024 float4 and not at 1025
