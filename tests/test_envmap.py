"""The `envmap` emitter (include/msk_gpu.h at msk_envmap_desc): image-based lighting, importance-sampled.

CPU: the restatement checks itself (envmap_ref.py), layout and exports, the two flatteners and the image readers (.hdr included),
the cumulative tables and the launch plan as stand-alone native programs.  GPU: the probes equal the fp32 restatement bit for
bit; a uniform image is the oracle's constant sky; rendered radiance under a non-uniform image meets float64 quadrature (the
Jacobian, the MIS density of the miss branch, the distribution, light selection); every execution variant makes the same film;
bad descriptors are refused; a group context renders the scene.

Standard errors measured on an MI355X (counter RNG, 64 pixels x 4096 spp, relative to the expectation, worst channel): see
EXPERIMENTS.md, "The envmap emitter"."""
import ctypes as C
import importlib
import os
import struct
import subprocess

import numpy as np
import pytest

import envmap_ref as E
import radiometry_ref as R
import test_launch_plan as LP
import test_table_placement as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
IDENTITY = np.eye(3, dtype=F)


def skew_rotation():
    """a rotation about the skew axis (1, 2, 3) by 0.7 rad (Rodrigues, in double, rounded to float)"""
    a = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    k = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return (np.eye(3) + np.sin(0.7) * k + (1 - np.cos(0.7)) * (k @ k)).astype(F)


ROTATIONS = {"identity": IDENTITY, "skew": skew_rotation()}


def images():
    """the four probe images, float32 [H, W, 3]: 1x1, 2x1, 3x5, and 16x8 with one texel 1e4 times the rest and one all-zero row"""
    rng = np.random.RandomState(5)
    big = rng.uniform(0.01, 0.05, (8, 16, 3)).astype(F)
    big[2, 11] = big[2, 11] * F(1e4)
    big[5] = 0
    return {"1x1": np.array([[[0.5, 0.4, 0.3]]], F), "2x1": np.array([[[0.25, 0.5, 0.125], [2.0, 1.0, 3.0]]], F),
            "3x5": rng.uniform(0, 2, (5, 3, 3)).astype(F), "16x8": big}


def env_spec(pixels, to_world=IDENTITY, scale=1.0, **kw):
    return dict({"type": "envmap", "pixels": np.asarray(pixels, F), "scale": scale, "to_world": np.asarray(to_world, F)}, **kw)


def restatements(hm, oracle, env, fetch=None):
    """(Env32, Env64, abi.EnvmapDesc, keep) of an env spec, through the mirror's flattener"""
    r2s = importlib.import_module("misaki-render_amd.rgb2spec")
    desc, keep = hm.envmap_desc(env, fetch or r2s.srgb_model_fetch)
    tex, wts = keep[0].reshape(desc.height, desc.width, 4), keep[1].reshape(desc.height, desc.width)
    _, d65 = hm.cie_tables()
    d65_scale = F(hm._radiance_desc(None, None, env.get("scale", 1.0))[1])
    rot = np.array(desc.to_world[:], F).reshape(3, 3)
    e32 = E.Env32(oracle, tex, wts, rot, (d65 * d65_scale).astype(F)) if oracle is not None else None
    return e32, E.Env64(tex, wts, rot, d65, d65_scale), desc, keep


def unit(v):
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(F)


def excluded(cell_a, cell_b):
    return (cell_a[0] != cell_b[0]) | (cell_a[1] != cell_b[1])


# ===================================================================================================== CPU
@pytest.mark.parametrize("rot", sorted(ROTATIONS))
@pytest.mark.parametrize("name", sorted(images()))
def test_restatement_checks_itself(hostmirror, oracle, name, rot):
    """(1) the float64 density integrates to 1; pdf(direction(sample(u))) is the sampler's pdf outside the stated rounding case."""
    e32, e64, desc, _ = restatements(hostmirror, oracle, env_spec(images()[name], ROTATIONS[rot]))
    # aligned with the cells the midpoint rule is exact up to rounding; a grid in (cos theta, phi) of the emitter's frame is not
    # aligned: a cell border cuts at most one node per line, 1 / 128 of a 16 x 8 cell's nodes in either direction
    d, dw, _, _ = e64.sphere_nodes(16 * desc.width, 16 * desc.height)
    assert abs(float((e64.pdf(d) * dw).sum()) - 1.0) < 1e-6           # (a rotation rounded to float is orthonormal within 1e-7)
    nz, nphi = 1024, 2048
    z, ph = np.meshgrid(1 - 2 * (np.arange(nz) + 0.5) / nz, 2 * np.pi * (np.arange(nphi) + 0.5) / nphi, indexing="ij")
    s = np.sqrt(1 - z * z)
    dirs = np.stack([s * np.sin(ph), z, -s * np.cos(ph)], -1) @ e64.R.T
    total = float(e64.pdf(dirs).sum() * 4 * np.pi / (nz * nphi))
    print("ENVMAP %s %s: integral of the float64 pdf over (cos theta, phi) = %.6f" % (name, rot, total))
    assert abs(total - 1.0) < 2.0 / 128
    # the float32 sampler against the float32 lookup
    u = np.random.RandomState(3).uniform(0, 1, (4096, 2)).astype(F)
    dirs, uv, pdf_s, cell_s = e32.sample(u)
    assert np.all(np.abs(np.linalg.norm(dirs.astype(np.float64), axis=1) - 1) < 1e-6) and np.all(pdf_s > 0)
    _, pdf_d, cell_d = e32.eval_dir(dirs, np.full((len(u), 4), 550, F))
    out = excluded(cell_s, cell_d)
    print("ENVMAP %s %s: %d of %d probe points change cell on the way back" % (name, rot, int(out.sum()), len(u)))
    assert out.mean() <= 1e-3
    if rot == "identity":          # R = 1: the local direction comes back exactly, so sin theta and the density do, bit for bit
        assert np.array_equal(pdf_s[~out].view(np.uint32), pdf_d[~out].view(np.uint32))
    else:                           # R^T (R d) is d within three roundings of terms below 1 per component and the 1e-7 by which the rounded
        # matrix is not orthonormal: 2^-22 absolute on sin theta, which is what the density divides by, plus the roundings after it
        sin_theta = np.sin(np.pi * uv[~out, 1].astype(np.float64))
        assert np.all(np.abs(pdf_s[~out].astype(np.float64) / pdf_d[~out] - 1) <= 2.0 ** -21 / sin_theta + 2.0 ** -21)
    # ... and the float64 side tells the same story as the float32 side
    assert np.allclose(e64.pdf(dirs.astype(np.float64))[~out], pdf_s[~out], rtol=1e-4)


def test_restatement_hand_checked_values(oracle):
    """(1) poles and the u seam on a 2x1 image of white texels (S = 1) with factors 1 and 3, emitter table 1: L is the bilinear
    interpolation of the factors; and a 1x3 image for the clamp at the poles."""
    inf = np.inf
    tex = np.array([[[0, 0, inf, 1], [0, 0, inf, 3]]], F)
    e = E.Env32(oracle, tex, np.array([[1, 3]], F), IDENTITY, np.ones(95, F))
    wl = np.full((1, 4), 500, F)
    assert list(e.cond[0]) == [0, 0.25, 1] and list(e.marg) == [0, 1]

    def at(d):
        u, v, st = e.dir_to_uv(np.array([d], F))
        return float(u[0]), float(v[0]), float(st[0]), float(e.radiance_uv(u, v, wl)[0, 0])
    assert at((0, 1, 0)) == (0.0, 0.0, 2.0 ** -24, 2.0)                 # the north pole: u = 0 is the seam, halfway between the texels
    u, v, st, l = at((0, -1, 0))
    assert (u, v, l) == (0.0, 1.0, 2.0)                                  # the south pole: v = 1 exactly, row H - 1
    assert at((0, 0, -1))[:2] == (0.0, 0.5) and at((0, 0, 1))[:2] == (0.5, 0.5) and at((1, 0, 0))[:2] == (0.25, 0.5) and at((-1, 0, 0))[:2] == (0.75, 0.5)
    assert at((1, 0, 0))[3] == 1.0 and at((-1, 0, 0))[3] == 3.0 and at((0, 0, 1))[3] == 2.0      # texel centres, and the inner border
    assert at((-1e-9, 0, -1))[0] == 0.0                                  # a tiny negative angle wraps to 1, which is 0
    u, _, _, l = at((-0.1, 0, -1))
    assert 0.98 < u < 1 and abs(l - (3 + (1 - 3) * (u * 2 - 0.5 - 1))) < 1e-6       # across the seam: from texel 1 towards texel 0
    # density: p = pmf * W * H / (2 pi^2 sin theta); the pole's sin theta is the epsilon
    _, pdf, cell = e.eval_dir(np.array([(1, 0, 0), (-1, 0, 0), (0, 1, 0)], F), np.repeat(wl, 3, 0))
    assert np.allclose(pdf[:2], [0.25 * 2 / (2 * np.pi ** 2), 0.75 * 2 / (2 * np.pi ** 2)], rtol=1e-6) and list(cell[0]) == [0, 1, 0]
    assert np.isclose(pdf[2], 0.25 * 2 / (2 * np.pi ** 2 * 2.0 ** -24), rtol=1e-6)
    # sampling: u.x below 0.25 lands in texel 0, reused; borders and the ends
    d, uv, pdf, cell = e.sample(np.array([(0.125, 0.5), (0.25, 0.5), (0.0, 0.0), (1 - 2.0 ** -24, 1 - 2.0 ** -24)], F))
    assert list(cell[0]) == [0, 1, 0, 1] and np.allclose(uv[:3], [(0.25, 0.5), (0.5, 0.5), (0, 0)]) and uv[3, 0] <= 1 and uv[3, 1] <= 1      # ((1 + du) / 2 rounds to 1)
    assert np.allclose(d[0], (1, 0, 0), atol=1e-6) and np.allclose(d[1], (0, 0, 1), atol=1e-6) and np.allclose(d[2], (0, 1, 0), atol=1e-6)
    # three rows: v clamps (no wrap from the north pole to the south pole)
    tex3 = np.array([[[0, 0, inf, 1]], [[0, 0, inf, 2]], [[0, 0, inf, 8]]], F)
    e3 = E.Env32(oracle, tex3, np.array([[1], [0], [1]], F), IDENTITY, np.ones(95, F))
    assert float(e3.radiance_uv(np.zeros(1, F), np.zeros(1, F), wl)[0, 0]) == 1.0 and float(e3.radiance_uv(np.zeros(1, F), np.ones(1, F), wl)[0, 0]) == 8.0
    assert list(e3.marg) == [0, 0.5, 0.5, 1] and float(e3.pdf_cell(np.array([0]), np.array([1]), np.ones(1, F))[0]) == 0.0      # the empty row


def test_layout_and_exports(abi, tmp_path):
    """(2)"""
    src = tmp_path / "off.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "msk_gpu.h"\nint main(){printf("%zu %zu %zu %zu %zu %zu %d %d\\n",'
                   'sizeof(msk_envmap_desc),offsetof(msk_envmap_desc,height),offsetof(msk_envmap_desc,texels),offsetof(msk_envmap_desc,weights),'
                   'offsetof(msk_envmap_desc,to_world),sizeof(msk_emitter_desc),MSK_EMITTER_ENVMAP,MSK_ABI_VERSION);return 0;}\n')
    exe = tmp_path / "off"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    d = abi.EnvmapDesc
    assert got == [C.sizeof(d), d.height.offset, d.texels.offset, d.weights.offset, d.to_world.offset, C.sizeof(abi.EmitterDesc), abi.MSK_EMITTER_ENVMAP, abi.MSK_ABI_VERSION]
    assert got[0] == 64 and got[6] == 2 and got[7] == 8
    import __graft_entry__ as ge
    ge.build_gpu_library()
    lib = C.CDLL(abi.LIB_PATH)
    for name in ("msk_gpu_scene_create_env", "msk_gpu_env_eval", "msk_gpu_env_sample"):
        assert name in abi.EXPORTS and getattr(lib, name) is not None
    blob = open(abi.LIB_PATH, "rb").read()
    for k in (b"k_shade_gen_e", b"k_wavefront_e", b"k_wavefront_h_e", b"k_path_serial_e", b"k_env_probe"):
        assert k in blob, k


def host_library():
    import __graft_entry__ as ge
    ge.build_gpu_library()
    ge.build_host_library()
    return importlib.import_module("misaki-render_amd.hostlib")


def plane_meshes(hm, bsdf=None, size=50.0, reflectance=(0.6, 0.5, 0.4)):
    """one large horizontal plane through the origin, facing +y"""
    s = float(size)
    return [hm.MeshSpec("plane", [((-s, 0, s), (s, 0, s), (s, 0, -s), (-s, 0, -s))], reflectance, bsdf=bsdf)]


PLANE_CAMERA = dict(fov=20.0, near=0.1, far=1000.0, origin=(0, 3, 8), target=(0, 0, 0), up=(0, 1, 0))


def test_the_two_flatteners_agree(hostmirror, abi, tmp_path):
    """(3) the mirror writes the PFM and the <emitter type="envmap">; the C++ plugin reads them back into the same two descriptors,
    byte for byte (both sides fetch coefficients from the host library's table)."""
    hostlib = host_library()
    img = images()["3x5"].copy()
    img[1, 1] = 0
    img[2, 0] = [-1, 0.5, np.nan]                                      # negative components and NaNs count as 0
    img[4, 2] = img[0, 0]                                              # an equal colour: fetched once
    for first in (False, True):
        env = env_spec(img, skew_rotation(), scale=2.5, first=first)
        d = tmp_path / ("first" if first else "last")
        xml = hostmirror.write_scene_xml(plane_meshes(hostmirror), str(d), 16, 16, 1, camera=PLANE_CAMERA, env=env)
        assert os.path.exists(d / "textures" / "envmap.pfm") and 'type="envmap"' in open(xml).read()
        h = hostlib.HostScene(xml).flatten()
        m = hostmirror.flatten(plane_meshes(hostmirror), 16, 16, camera=PLANE_CAMERA, env=env, coeff_lookup=hostlib.srgb_model_fetch)
        assert h.envmap is not None and m.envmap is not None
        a, b = h.envmap, m.envmap
        assert (a.width, a.height) == (b.width, b.height) == (3, 5) and list(a.to_world) == list(b.to_world) == [float(x) for x in skew_rotation().reshape(-1)]
        for field, n in (("texels", 60), ("weights", 15)):
            x, y = np.ctypeslib.as_array(getattr(a, field), (n,)), np.ctypeslib.as_array(getattr(b, field), (n,))
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), field
        tex = np.ctypeslib.as_array(b.texels, (60,)).reshape(5, 3, 4)
        assert list(tex[1, 1]) == [0, 0, 0, 0] and tex[0, 0, 3] == img[0, 0].max() * 2 and np.array_equal(tex[4, 2], tex[0, 0]) and tex[2, 0, 3] == 1.0
        wts = np.ctypeslib.as_array(b.weights, (15,)).reshape(5, 3)
        assert np.all(wts > 0) and np.all(np.isfinite(wts))            # 3x3 neighbourhoods: a black texel beside bright ones has weight
        assert h.desc.n_emitters == m.desc.n_emitters == 1
        ea, eb = h.desc.emitters[0], m.desc.emitters[0]
        assert bytes(ea) == bytes(eb) and (eb.type, eb.mesh_id, eb.radiance_regular) == (abi.MSK_EMITTER_ENVMAP, -1, 0)
        assert list(eb.radiance) == [0, 0, np.inf] and eb.d65_scale == F(F(2.5) * (F(1) / F(10568)))
    # `constant` keeps ignoring a filename
    text = open(xml).read()
    start, end = text.index('<emitter type="envmap">'), text.index('</emitter>', text.index('<emitter type="envmap">')) + len('</emitter>')
    (tmp_path / "const.xml").write_text(text[:start] + '<emitter type="constant"><string name="filename" value="textures/envmap.hdr"/></emitter>' + text[end:])
    os.makedirs(tmp_path / "textures", exist_ok=True)
    h = hostlib.HostScene(str(tmp_path / "const.xml")).flatten()
    assert h.envmap is None and h.desc.emitters[0].type == abi.MSK_EMITTER_CONSTANT


def test_flatten_refuses_a_to_world_that_is_no_rotation(hostmirror, tmp_path):
    """(3) at flatten, in the plugin and in the mirror, as at scene creation: a mirror, a scale, a shear, a translation"""
    hostlib = host_library()
    rot4 = np.eye(4, dtype=F)
    rot4[:3, :3] = skew_rotation()
    moved = rot4.copy()
    moved[0, 3] = 1
    bad = {"mirror": np.diag([1, 1, -1]).astype(F), "scale": (2 * np.eye(3)).astype(F), "shear": np.array([[1, 0.1, 0], [0, 1, 0], [0, 0, 1]], F), "translation": moved}
    good = hostmirror.write_scene_xml(plane_meshes(hostmirror), str(tmp_path), 16, 16, 1, camera=PLANE_CAMERA, env=env_spec(images()["2x1"], rot4))
    assert hostlib.HostScene(good).flatten().envmap is not None
    text = open(good).read()
    start, end = text.index('<matrix value="', text.index('type="envmap"')), text.index('"/>', text.index('<matrix value="', text.index('type="envmap"')))
    for name, m in bad.items():
        with pytest.raises(ValueError) as e:
            hostmirror.flatten(plane_meshes(hostmirror), 16, 16, camera=PLANE_CAMERA, env=env_spec(images()["2x1"], m))
        assert "to_world must be a rotation" in str(e.value), name
        m4 = np.eye(4)
        m4[:m.shape[0], :m.shape[1]] = m
        (tmp_path / (name + ".xml")).write_text(text[:start] + '<matrix value="' + " ".join("%.9g" % x for x in m4.reshape(-1)) + text[end:])
        with pytest.raises(hostlib.HostError) as e:
            hostlib.HostScene(str(tmp_path / (name + ".xml"))).flatten()
        assert "to_world must be a rotation" in str(e.value) and "envmap.pfm" in str(e.value), name


def rgbe_encode(rgbe, rle):
    """uint8 [H, W, 4] -> the scanline bytes of a Radiance file: flat, or run-length encoded per channel (8 <= W < 32768) with a
    run wherever at least three equal bytes follow each other and literal stretches of at most 128 otherwise"""
    h, w = rgbe.shape[:2]
    if not rle:
        return rgbe.tobytes()
    out = bytearray()
    for y in range(h):
        out += bytes([2, 2, w >> 8, w & 255])
        for c in range(4):
            row, x = rgbe[y, :, c], 0
            while x < w:
                run = 1
                while x + run < w and run < 127 and row[x + run] == row[x]:
                    run += 1
                if run >= 3:
                    out += bytes([128 + run, int(row[x])])
                    x += run
                    continue
                lit = x
                while lit < w and lit - x < 128 and not (lit + 2 < w and row[lit] == row[lit + 1] == row[lit + 2]):
                    lit += 1
                lit = max(lit, x + 1)
                out += bytes([lit - x]) + row[x:lit].tobytes()
                x = lit
    return bytes(out)


def rgbe_decode(rgbe):
    m, e = rgbe[..., :3].astype(np.float64), rgbe[..., 3].astype(np.int64)
    return np.where(e[..., None] == 0, 0.0, (m + 0.5) * np.ldexp(1.0, e - 136)[..., None]).astype(F)


def test_hdr_reader(hostmirror, tmp_path):
    """(3) Radiance RGBE, flat and run-length encoded, W = 8 and W = 40, against an encoder written here, against a PFM of the same
    pixels, and each refusal by name."""
    hostlib = host_library()
    rng = np.random.RandomState(9)
    for w in (8, 40):
        px = rng.randint(0, 256, (5, w, 4)).astype(np.uint8)
        px[..., 3] = rng.randint(120, 140, (5, w))
        px[1, :, :] = px[1, 0, :]                                       # a row of one colour: pure runs
        px[2, 2:7, 1] = 7                                               # a run inside literals
        px[3, 3] = [200, 100, 50, 0]                                    # exponent 0: black whatever the mantissas say
        want = rgbe_decode(px)
        assert want[3, 3].tolist() == [0, 0, 0] and want[0, 0, 0] == (px[0, 0, 0] + 0.5) * 2.0 ** (int(px[0, 0, 3]) - 136)
        hostmirror.write_pfm(str(tmp_path / ("same%d.pfm" % w)), want)
        for rle in (False, True):
            p = tmp_path / ("%s%d.hdr" % ("rle" if rle else "flat", w))
            body = rgbe_encode(px, rle)
            assert rle == (len(body) != px.size)
            p.write_bytes(b"#?RADIANCE\n# a comment\nFORMAT=32-bit_rle_rgbe\nEXPOSURE=1.0\n\n-Y 5 +X %d\n" % w + body)
            got = hostlib.read_image(p)
            assert got.shape == (5, w, 3) and np.array_equal(got.view(np.uint32), want.view(np.uint32)), (w, rle)
            assert np.array_equal(got, hostlib.read_image(tmp_path / ("same%d.pfm" % w)))
    good = b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y 5 +X 40\n"
    (tmp_path / "rgbe.hdr").write_bytes(b"#?RGBE\n\n-Y 5 +X 40\n" + px.tobytes())                  # the other magic, no FORMAT line
    assert np.array_equal(hostlib.read_image(tmp_path / "rgbe.hdr"), want)
    bad_len = bytearray(rgbe_encode(px, True))
    bad_len[3] = 41
    old = px.copy()
    old[0, 5, :3] = 1
    cases = {"xyze.hdr": (b"#?RADIANCE\nFORMAT=32-bit_rle_xyze\n\n-Y 5 +X 40\n" + px.tobytes(), "32-bit_rle_xyze"),
             "flipped.hdr": (b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n+Y 5 +X 40\n" + px.tobytes(), "+Y 5 +X 40"),
             "columns.hdr": (b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n+X 40 -Y 5\n" + px.tobytes(), "+X 40 -Y 5"),
             "short.hdr": (good + px.tobytes()[:-3], "truncated"),
             "shortrle.hdr": (good + rgbe_encode(px, True)[:-2], "truncated"),
             "length.hdr": (good + bytes(bad_len), "has length 41"),
             "oldrle.hdr": (good + old.tobytes(), "old-style run-length"),
             "header.hdr": (b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n", "header")}
    for name, (content, text) in cases.items():
        (tmp_path / name).write_bytes(content)
        with pytest.raises(hostlib.HostError) as e:
            hostlib.read_image(tmp_path / name)
        assert name in str(e.value) and text in str(e.value), str(e.value)
    # the plugin reads a .hdr through the file resolver
    xml = hostmirror.write_scene_xml(plane_meshes(hostmirror), str(tmp_path), 16, 16, 1, camera=PLANE_CAMERA, env=env_spec(np.ones((1, 1, 3), F)))
    (tmp_path / "hdr.xml").write_text(open(xml).read().replace("textures/envmap.pfm", "rle40.hdr"))
    h = hostlib.HostScene(str(tmp_path / "hdr.xml")).flatten()
    assert (h.envmap.width, h.envmap.height) == (40, 5)
    assert np.array_equal(np.ctypeslib.as_array(h.envmap.texels, (800,)).reshape(5, 40, 4)[..., 3], want.max(-1) * 2)


def test_cumulative_tables_native(tmp_path):
    """(4) csrc/msk_envmap.h as a stand-alone program, plainly and under AddressSanitizer + UBSan"""
    src = os.path.join(ROOT, "tests", "native", "envmap_cdf_check.cpp")
    for tag, flags in (("plain", ["-O2"]), ("san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = str(tmp_path / ("envmap_cdf_check_" + tag))
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + flags + ["-o", exe, src])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stdout.split() == ["cases", "35"], r.stdout[-2000:] + r.stderr[-2000:]


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("launch_plan_envmap") / "launch_plan_envmap_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", out, os.path.join(ROOT, "tests", "native", "launch_plan_envmap_check.cpp")])
    return out


@pytest.mark.parametrize("knobs", LP.KNOB_SETS, ids=lambda k: ",".join(f"{a}={b}" for a, b in k.items()) or "defaults")
def test_plan_with_an_envmap(plan_exe, knobs):
    """(5) has_envmap selects SHADE_ENVMAP everywhere and changes nothing else; without it the plan is what it was"""
    env = {k: v for k, v in os.environ.items() if not k.startswith("MSK_")}
    env.update(knobs)
    r = subprocess.run([plan_exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    assert r.stdout.split() == ["cases", str(7 * 64 * 4 * len(LP.REGION_SIZES) * len(LP.LDS))]


# ===================================================================================================== GPU: the probes
def probe_inputs(e32, rng, n=4096):
    """random numbers with the cell borders of both tables, 0 and 1 - 2^-24; directions with the poles, the seam and the axes"""
    u = rng.uniform(0, 1, (n, 2)).astype(F)
    edge = np.concatenate([e32.marg, e32.cond.reshape(-1), [0, 1 - 2.0 ** -24, 0.5]]).astype(F)
    edge = np.minimum(edge, F(1 - 2.0 ** -24))
    k = min(len(edge), n // 4)
    u[:k, 1] = edge[:k]
    u[k:2 * k, 0] = edge[:k]
    u[2 * k:2 * k + 4] = [(0, 0), (1 - 2.0 ** -24, 1 - 2.0 ** -24), (0, 1 - 2.0 ** -24), (1 - 2.0 ** -24, 0)]
    d = unit(rng.normal(size=(n, 3)))
    crafted = [(0, 1, 0), (0, -1, 0), (0, 0, -1), (0, 0, 1), (1, 0, 0), (-1, 0, 0), (-1e-9, 0, -1), (1e-9, 0, -1), (-1e-4, 0.5, -1), (0, 1, 1e-30), (1e-20, -1, 0)]
    local = unit(crafted)
    d[:len(local)] = (local.astype(np.float64) @ e32.R.astype(np.float64).T).astype(F)      # poles and seam of the emitter's frame
    d[len(local):2 * len(local)] = local
    wl = rng.uniform(360, 830, (n, 4)).astype(F)
    return u, d, wl


@pytest.mark.gpu
@pytest.mark.parametrize("rot", sorted(ROTATIONS))
@pytest.mark.parametrize("name", sorted(images()))
def test_probes_equal_the_restatement_bit_for_bit(gpu_ctx, hostmirror, oracle, abi, name, rot):
    """(6) msk_gpu_env_sample and msk_gpu_env_eval run the device functions the shading kernels call."""
    env = env_spec(images()[name], ROTATIONS[rot], scale=1.5)
    e32, _, _, _ = restatements(hostmirror, oracle, env)
    flat = hostmirror.flatten(plane_meshes(hostmirror), 16, 16, camera=PLANE_CAMERA, env=env)
    u, d, wl = probe_inputs(e32, np.random.RandomState(17))
    g = abi.Scene(gpu_ctx, flat)
    gd, guv, gpdf = g.env_sample(u)
    grad, gp = g.env_eval(d, wl)
    g.close()
    rd, ruv, rpdf, _ = e32.sample(u)
    rrad, rp, _ = e32.eval_dir(d, wl)
    bits = lambda a: np.ascontiguousarray(a, F).view(np.uint32)
    for what, a, b in (("uv", guv, ruv), ("direction", gd, rd), ("sampled pdf", gpdf, rpdf), ("radiance", grad, rrad), ("pdf", gp, rp)):
        bad = (bits(a) != bits(b)).reshape(len(a), -1).any(-1)
        assert not bad.any(), (what, int(bad.sum()), np.asarray(a)[bad][:3], np.asarray(b)[bad][:3])
    assert np.all(gpdf > 0) and np.all(np.isfinite(grad)) and np.all(np.isfinite(gp))


# ===================================================================================================== GPU: renders
def pcg(abi, **kw):
    return abi.render_params(rng_mode=abi.MSK_RNG_PCG_BLOCK, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("hide", [0, 1])
def test_uniform_image_is_the_constant_sky(gpu_ctx, oracle, hostmirror, abi, hide):
    """(7) texels (0.5, 0.4, 0.3), so w = 1: at max_depth = 1 the film is the oracle's film of the scene with a constant emitter of
    that colour, bit for bit, in both RNG modes.  (The Cornell box without its ceiling and back wall: part of the film sees the sky.)"""
    meshes = [m for m in hostmirror.cbox_meshes() if m.name not in ("cbox_ceiling", "cbox_back")]
    img = np.broadcast_to(np.array([0.5, 0.4, 0.3], F), (3, 4, 3))
    fe = hostmirror.flatten(meshes, 48, 48, env=env_spec(img, skew_rotation()))
    fc = hostmirror.flatten(meshes, 48, 48, env={"radiance": (0.5, 0.4, 0.3)})
    assert fe.desc.emitters[fe.desc.n_emitters - 1].type == abi.MSK_EMITTER_ENVMAP and fc.desc.emitters[fc.desc.n_emitters - 1].type == abi.MSK_EMITTER_CONSTANT
    g, o = abi.Scene(gpu_ctx, fe), oracle.scene(fc)
    for prm in (abi.render_params(spp=4, seed=3, max_depth=1, hide_emitters=hide), pcg(abi, spp=2, seed=3, max_depth=1, hide_emitters=hide)):
        film, st = g.render(prm)
        ref, rst = o.render(prm, threads=8)
        assert st.samples == rst.samples == 48 * 48 * prm.spp
        assert np.array_equal(film.view(np.uint32), ref.view(np.uint32)), (hide, prm.rng_mode, float(np.abs(film - ref).max()))
        assert (film[..., :3].max() > 0) or hide                       # the sky and the luminaire are in view
    g.close(); o.close()


def lit_image():
    """16x8: a hot block above the horizon, a dim gradient elsewhere"""
    j, i = np.meshgrid(np.arange(8), np.arange(16), indexing="ij")
    img = np.stack([0.02 + 0.004 * i, 0.03 + 0.005 * j, 0.05 - 0.002 * i], -1).astype(F)
    img[1:3, 9:12] = np.array([1.5, 1.2, 0.9], F)
    return img


# (eta, k and the specular reflectance of the conductor are `uniform` spectra: constants over the wavelengths, as the closed form needs)
FLOORS = {"diffuse": (None, IDENTITY),
          "roughconductor": ({"type": "roughconductor", "alpha": 0.3, "eta": 0.2, "k": 3.9, "specular_reflectance": 1.0}, IDENTITY),
          "twosided_rotated": ({"type": "diffuse", "twosided": True}, skew_rotation())}
W48, CROP = 48, (20, 28)           # the film, and the first pixel of the 8x8 crop the tests look at (it sees the plane near the origin)


def crop_pixels():
    return np.array([(x, y) for y in range(CROP[1], CROP[1] + 8) for x in range(CROP[0], CROP[0] + 8)], np.int32)


def sigmoid_spectrum(coeff, scale=1.0):
    c0, c1, c2 = (float(c) for c in coeff)
    if np.isinf(c2):
        return R.constant(scale * (1.0 if c2 > 0 else 0.0))

    def fn(lam):
        x = (c0 * lam + c1) * lam + c2
        return scale * (0.5 + x / (2.0 * np.sqrt(1.0 + x * x)))
    return R.Spectrum(fn)


def expected_plane_xyz(flat, e64, floor, area=None, nodes=(1024, 512)):
    """float64: the mean over the crop of E[XYZ] of a camera sample at max_depth = 2 — the plane lit by the sky (and by `area`, a
    (vertices, Spectrum) emitter the sky does not shine through), seen directly.  Diffuse: rho / pi * irradiance, the same for every
    pixel.  Rough conductor (GGX, isotropic, eta and k constant over the spectrum): F D G / (4 cos_i) integrated against the sky per
    camera direction, on a 6 x 6 Gauss-Legendre rule over the crop."""
    n = np.array([0.0, 1.0, 0.0])
    cie = np.array(flat.desc.cie1931_xyz[:285], np.float64)
    b = flat.desc.bsdfs[0]
    if floor != "roughconductor":
        rho = sigmoid_spectrum(b.reflectance[:], b.reflectance_scale / np.pi)
        c = e64.texel_moments(lambda d: np.maximum(d @ n, 0.0), *nodes)
        sky = e64.lit_spectrum(c)
        if area is None:
            return R.expected_xyz(sky * rho, cie)
        verts, le = area
        t, w = R.gauss_legendre(4)
        yy, xx = np.meshgrid(CROP[1] + 8 * t, CROP[0] + 8 * t, indexing="ij")
        o, d = R.camera_ray(flat.desc, xx, yy)
        geom = float((w[:, None] * w[None, :] * R.polygon_irradiance(R.hit_plane(o, d, (0, 0, 0), n), n, verts)).sum())
        return R.expected_xyz(R.Spectrum(lambda lam: (sky(lam) + le(lam) * geom) * rho(lam), sky.breaks), cie)
    t, w = R.gauss_legendre(6)
    yy, xx = np.meshgrid(CROP[1] + 8 * t, CROP[0] + 8 * t, indexing="ij")
    return (conductor_xyz(flat, e64, xx, yy, nodes) * (w[:, None] * w[None, :])[..., None]).sum((0, 1))


def conductor_xyz(flat, e64, xx, yy, nodes):
    """E[XYZ] of a camera sample through the film positions (xx, yy) that sees the rough-conductor plane under the sky -> [..., 3]"""
    n = np.array([0.0, 1.0, 0.0])
    cie = np.array(flat.desc.cie1931_xyz[:285], np.float64)
    b = flat.desc.bsdfs[0]
    alpha, eta, k = float(b.alpha_u), float(b.eta.scale), float(b.k.scale)
    _, dirs = R.camera_ray(flat.desc, xx, yy)
    out = []
    for q in dirs.reshape(-1, 3):
        wi = -q
        ci = float(wi @ n)

        def g(d):
            co = d @ n
            h = d + wi
            h = h / np.linalg.norm(h, axis=-1, keepdims=True)
            hz = h @ n
            dist = 1.0 / (np.pi * alpha * alpha * ((1 - hz * hz) / (alpha * alpha) + hz * hz) ** 2)
            g1 = lambda c: 2.0 / (1.0 + np.sqrt(1.0 + alpha * alpha * (1 - c * c) / (c * c)))
            with np.errstate(divide="ignore", invalid="ignore"):
                f = R.fresnel_conductor(h @ wi, eta, k) * dist * g1(ci) * g1(co) / (4.0 * ci)
            return np.where(co > 0, f, 0.0)
        out.append(R.expected_xyz(e64.lit_spectrum(e64.texel_moments(g, *nodes)), cie))
    return np.array(out).reshape(np.shape(xx) + (3,))


def film_row_weights(desc, n, per=64):
    """the filter weight a sample at film coordinate x leaves in the n pixels of a row (imageblock.cpp:83-114 with the film's own
    table: weight lut[min((int) |p - (x - 0.5)| * 32 / radius, 32)] in pixel p), on a midpoint grid of `per` points per pixel"""
    lut, scale = np.array(desc.film.filter_lut[:], np.float64), 32.0 / float(desc.film.filter_radius)
    x = (np.arange(n * per) + 0.5) / per
    idx = np.minimum((np.abs(np.arange(n)[:, None] - (x[None, :] - 0.5)) * scale).astype(np.int64), 32)
    return x, lut[idx].sum(0)


def lagrange(t, x):
    """[len(x), len(t)]: the Lagrange basis polynomials of the nodes t at the points x"""
    out = np.ones((len(x), len(t)))
    for k in range(len(t)):
        for l in range(len(t)):
            if l != k:
                out[:, k] *= (x - t[l]) / (t[k] - t[l])
    return out


def expected_film_xyz(flat, e64, floor, size, m=8, nodes=(1024, 512)):
    """float64: what the film's sum of X, Y, Z over its sum of weights estimates — the mean of the per-position expectation over
    the film, weighted with the filter weight a sample at that position leaves inside the film (samples near the border leave
    part of theirs outside).  The two diffuse floors have one expectation everywhere.  The conductor's is smooth in the film
    position: it is evaluated on an m x m Gauss-Legendre grid over the film, interpolated by the grid's polynomial and integrated
    against the (separable, jagged) filter weight on 64 points per pixel.
    -> (expectation [3], effective samples / samples = (sum w)^2 / (N sum w^2) of that weight)"""
    x, wx = film_row_weights(flat.desc, size)
    n_eff = (wx.mean() ** 2 / (wx * wx).mean()) ** 2                  # the weight is wx(x) wx(y) on a square film
    if floor != "roughconductor":
        return expected_plane_xyz(flat, e64, floor, nodes=nodes), n_eff
    t, _ = R.gauss_legendre(m, 0.0, float(size))
    yy, xx = np.meshgrid(t, t, indexing="ij")
    v = conductor_xyz(flat, e64, xx, yy, nodes)                        # [y node, x node, 3]
    a = (wx @ lagrange(t, x)) / wx.sum()
    return np.einsum("j,k,jkc->c", a, a, v), n_eff


def sampled_mean(g, abi, floor, expected, **kw):
    """mean XYZ over the crop's samples and its standard error from the per-sample values; spp doubles from 4096 until the
    standard error is at most 0.5 % of the expectation (four doublings at the most)"""
    spp = 4096
    for _ in range(5):
        xyz, _ = g.sample_pixels(abi.render_params(spp=spp, seed=7, max_depth=2, **kw), crop_pixels())
        v = xyz.reshape(-1, 3).astype(np.float64)
        mean, se = v.mean(0), v.std(0, ddof=1) / np.sqrt(len(v))
        print("ENVMAP %s spp %d: expected %s mean %s se/|E| %s dev/|E| %s" % (floor, spp, expected, mean, se / expected, (mean - expected) / expected))
        if np.all(se <= 5e-3 * expected):
            return mean, se, v.std(0, ddof=1)
        spp *= 2
    raise AssertionError("the standard error stays above 0.5 %% of the expectation: %s" % (se / expected,))


def plane_scene(hm, floor, extra=(), size=W48):
    bsdf, rot = FLOORS[floor]
    env = env_spec(lit_image(), rot, scale=3.0)
    return hm.flatten(plane_meshes(hm, bsdf) + list(extra), size, size, camera=PLANE_CAMERA, env=env), env


@pytest.mark.gpu
@pytest.mark.parametrize("floor", sorted(FLOORS))
def test_rendered_radiance_meets_the_quadrature(gpu_ctx, hostmirror, abi, floor):
    """(8) counter RNG through msk_gpu_sample_pixels: |mean - expectation| <= 6 standard errors + 1e-3 of the expectation (the
    quadrature and fp32 allowance of test_radiometry_closed_form.py).  A wrong Jacobian, a wrong MIS density on the miss branch or
    a biased distribution each move the mean by per cents."""
    flat, env = plane_scene(hostmirror, floor)
    _, e64, _, _ = restatements(hostmirror, None, env)
    expected = expected_plane_xyz(flat, e64, floor)
    coarse = expected_plane_xyz(flat, e64, floor, nodes=(512, 256))
    assert np.all(np.abs(coarse - expected) <= 2e-4 * expected), (coarse, expected)      # the quadrature has converged
    g = abi.Scene(gpu_ctx, flat)
    mean, se, _ = sampled_mean(g, abi, floor, expected)
    g.close()
    assert np.all(np.abs(mean - expected) <= 6 * se + 1e-3 * expected), ((mean - expected) / expected, se / expected)


def test_film_expectation_converges(hostmirror):
    """the conductor's film expectation: the 8 x 8 grid at 1024 x 512 sky nodes against 6 x 6 at 512 x 256, and the effective
    sample count the 2-pixel Gaussian leaves on a 32 x 32 film"""
    flat, env = plane_scene(hostmirror, "roughconductor", size=32)
    _, e64, _, _ = restatements(hostmirror, None, env)
    fine, n_eff = expected_film_xyz(flat, e64, "roughconductor", 32)
    coarse, _ = expected_film_xyz(flat, e64, "roughconductor", 32, m=6, nodes=(512, 256))
    print("ENVMAP film expectation fine %s coarse %s effective samples / samples %.4f" % (fine, coarse, n_eff))
    assert np.all(np.abs(coarse - fine) <= 2e-4 * fine), (coarse, fine)
    assert 0.8 < n_eff < 1.0


@pytest.mark.gpu
@pytest.mark.parametrize("floor", sorted(FLOORS))
def test_film_in_pcg_block_mode_meets_the_quadrature(gpu_ctx, hostmirror, abi, floor):
    """(8) MSK_RNG_PCG_BLOCK (k_path_serial_e), one block per film, through the film, on the three floors: the film's sum of X, Y, Z
    over its sum of weights against expected_film_xyz.  The film holds no per-sample values, so the standard error is put together
    from what can be measured: the per-sample deviation within a pixel, in counter mode on the same scene (the root of the mean
    over all 1024 pixels of the per-pixel variance), over the root of the effective sample count of the filter-weighted mean,
    (sum w)^2 / sum w^2 of the weights the samples leave inside the film — computed from the film's filter table, not assumed."""
    flat, env = plane_scene(hostmirror, floor, size=32)
    _, e64, _, _ = restatements(hostmirror, None, env)
    expected, n_eff = expected_film_xyz(flat, e64, floor, 32)
    g = abi.Scene(gpu_ctx, flat)
    px = np.array([(x, y) for y in range(32) for x in range(32)], np.int32)
    xyz, _ = g.sample_pixels(abi.render_params(spp=64, seed=9, max_depth=2), px)
    sigma = np.sqrt(xyz.astype(np.float64).var(1, ddof=1).mean(0))
    spp = 256
    film, st = g.render(pcg(abi, spp=spp, seed=7, max_depth=2))
    g.close()
    assert st.samples == 32 * 32 * spp
    f = film.astype(np.float64)
    mean = f[..., :3].sum((0, 1)) / f[..., 4].sum()
    se = sigma / np.sqrt(n_eff * st.samples)
    print("ENVMAP film %s: expected %s mean %s se/|E| %s dev/|E| %s effective samples / samples %.4f" % (
        floor, expected, mean, se / expected, (mean - expected) / expected, n_eff))
    assert np.all(se <= 5e-3 * expected)
    assert np.all(np.abs(mean - expected) <= 6 * se + 1e-3 * expected)


@pytest.mark.gpu
def test_envmap_plus_one_area_light(gpu_ctx, hostmirror, abi):
    """(9) n_emitters = 2 on the diffuse plane: a small square lamp high above the crop, under a sky whose two top rows are black,
    so that the lamp hides no lit part of the sky from the plane.  The same criterion: this is the light-selection factor."""
    lamp = [(0.5, 10, -0.5), (0.5, 10, 0.5), (-0.5, 10, 0.5), (-0.5, 10, -0.5)]                   # wound to face down, as the cbox luminaire
    img = lit_image()
    img[0:2] = 0
    env = env_spec(img, IDENTITY, scale=3.0)
    meshes = plane_meshes(hostmirror) + [hostmirror.MeshSpec("lamp", [tuple(lamp)], hostmirror.LUMINAIRE, radiance=(40, 30, 20))]
    for first in (False, True):
        flat = hostmirror.flatten(meshes, W48, W48, camera=PLANE_CAMERA, env=dict(env, first=first))
        d = flat.desc
        assert d.n_emitters == 2 and d.emitters[0 if first else 1].type == abi.MSK_EMITTER_ENVMAP
        _, e64, _, _ = restatements(hostmirror, None, env)
        ea = d.emitters[1 if first else 0]
        le = R.srgb_d65(ea.radiance[:], np.array(d.d65[:95], np.float64), ea.d65_scale)
        expected = expected_plane_xyz(flat, e64, "diffuse", area=(np.array(lamp, np.float64), le))
        sky_only = expected_plane_xyz(flat, e64, "diffuse")
        assert np.all(sky_only < 0.8 * expected) and np.all(sky_only > 0.2 * expected)           # both lights matter
        g = abi.Scene(gpu_ctx, flat)
        mean, se, _ = sampled_mean(g, abi, "sky + lamp, envmap %s" % ("first" if first else "last"), expected)
        g.close()
        assert np.all(np.abs(mean - expected) <= 6 * se + 1e-3 * expected), ((mean - expected) / expected, se / expected)


SPLIT, FUSED_PART, FUSED_ALL, ANY = "split", "fused part", "fused all", "any"
KNOBS = ("MSK_FUSED", "MSK_SORT", "MSK_STREAMS", "MSK_FUSED_HBM", "MSK_FUSED_TAIL_PCT", "MSK_BVH_BUILD", "MSK_WIDE_BVH", "MSK_QUANT_BVH", "MSK_LDS_SCENE_KB")
# the knob lists of test_bitmap_texture.py
LDS_VARIANTS = [({}, ANY), ({"MSK_FUSED": "1"}, FUSED_ALL), ({"MSK_SORT": "0", "MSK_STREAMS": "1"}, ANY), ({"MSK_FUSED_TAIL_PCT": "50"}, FUSED_PART),
                ({"MSK_BVH_BUILD": "gpu"}, ANY), ({"MSK_WIDE_BVH": "8"}, ANY), ({"MSK_QUANT_BVH": "1"}, ANY),
                ({"MSK_LDS_SCENE_KB": "0", "MSK_FUSED": "1"}, SPLIT), ({"MSK_LDS_SCENE_KB": "0", "MSK_WIDE_BVH": "8"}, SPLIT),
                ({"MSK_LDS_SCENE_KB": "0", "MSK_QUANT_BVH": "1", "MSK_BVH_BUILD": "gpu"}, SPLIT)]
HBM_VARIANTS = [({"MSK_LDS_SCENE_KB": "0", "MSK_FUSED_HBM": "0"}, SPLIT), ({"MSK_LDS_SCENE_KB": "0"}, ANY),
                ({"MSK_LDS_SCENE_KB": "0", "MSK_FUSED_TAIL_PCT": "50"}, FUSED_PART), ({"MSK_LDS_SCENE_KB": "0", "MSK_FUSED": "1"}, FUSED_ALL)]
variant_id = lambda e: ",".join("%s=%s" % kv for kv in sorted(e.items())) or "defaults"


def variant_meshes(hm, pads=()):
    """the open Cornell box of the constant-sky test with a glossy ball, a glass ball and a bitmap floor: every branch of the
    envmap instantiations has work"""
    meshes = [m for m in hm.cbox_meshes() if m.name not in ("cbox_ceiling", "cbox_back")]
    floor = next(m for m in meshes if m.name == "cbox_floor")
    floor.bsdf = {"type": "diffuse", "texture": {"type": "bitmap", "pixels": np.random.RandomState(2).uniform(0.1, 0.9, (4, 4, 3)).astype(F), "scale": (3, 3)}}
    floor.texcoords = [((0, 0), (1, 0), (1, 1), (0, 1)) for _ in floor.faces]
    glass = hm.blob_mesh("glass", (370, 90, 170), 80, 5, 5, hm.WHITE, seed=2)
    glass.bsdf = {"type": "dielectric"}
    return meshes + [glass] + list(pads)


def variant_flat(hm, which, scale=40.0):
    env = env_spec(lit_image(), skew_rotation(), scale=scale)
    if which == "lds":
        return hm.flatten(variant_meshes(hm), 48, 48, env=env)
    filler = hm.blob_mesh("filler", (150, 420, 400), 60, 16, 16, hm.WHITE, seed=9)
    base = hm.flatten(variant_meshes(hm, [filler]), 48, 48, env=env)
    pads = T.faceless_pads(hm, T.SMALL_TABLES_F4 + 1 - T.table_plan(base)["small_f4"])
    return hm.flatten(variant_meshes(hm, [filler] + pads), 48, 48, env=env)


def test_variant_scenes_sit_where_the_tests_say(hostmirror):
    lds, hbm = T.table_plan(variant_flat(hostmirror, "lds")), T.table_plan(variant_flat(hostmirror, "hbm"))
    assert lds["lds_tables"] and lds["small_staged"]
    assert not hbm["lds_tables"] and not hbm["small_staged"] and hbm["small_f4"] == T.SMALL_TABLES_F4 + 1


@pytest.fixture(scope="module")
def variant_reference(gpu_ctx, hostmirror, abi):
    """the default variant's samples and films of the two scenes (no knob set): computed once, never changed"""
    saved = {k: os.environ.pop(k) for k in KNOBS if k in os.environ}
    out = {}
    try:
        for which in ("lds", "hbm"):
            flat = variant_flat(hostmirror, which)
            g = abi.Scene(gpu_ctx, flat)
            xyz, pos = g.sample_pixels(abi.render_params(spp=16, seed=5), crop_pixels())
            film, st = g.render(abi.render_params(spp=8, seed=5))
            serial, _ = g.render(pcg(abi, spp=2, seed=5))
            g.close()
            for a in (xyz, pos, film, serial):
                a.setflags(write=False)
            assert np.isfinite(film).all() and film[..., :3].max() > 0
            out[which] = dict(flat=flat, xyz=xyz, pos=pos, film=film, serial=serial, samples=st.samples)
    finally:
        os.environ.update(saved)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("which,env,expect", [("lds", e, x) for e, x in LDS_VARIANTS] + [("hbm", e, x) for e, x in HBM_VARIANTS],
                         ids=lambda v: variant_id(v) if isinstance(v, dict) else str(v).replace(" ", "_"))
def test_every_execution_variant(gpu_ctx, abi, variant_reference, monkeypatch, which, env, expect):
    """(10) films and samples byte-equal to the default variant's; msk_stats says which kernels made the film."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    want = variant_reference[which]
    g = abi.Scene(gpu_ctx, want["flat"])
    gx, gp = g.sample_pixels(abi.render_params(spp=16, seed=5), crop_pixels())
    film, st = g.render(abi.render_params(spp=8, seed=5))
    serial, _ = g.render(pcg(abi, spp=2, seed=5))
    g.close()
    got = "trace %d shade %d wavefront %d" % (st.launches_trace, st.launches_shade, st.launches_wavefront)
    print("ENVMAP variant %s %s: %s" % (which, variant_id(env), got))
    assert np.array_equal(gp.view(np.uint32), want["pos"].view(np.uint32))
    assert np.array_equal(gx.view(np.uint32), want["xyz"].view(np.uint32)), env
    assert np.array_equal(film.view(np.uint32), want["film"].view(np.uint32)), (env, float(np.abs(film - want["film"]).max()))
    assert np.array_equal(serial.view(np.uint32), want["serial"].view(np.uint32)), env
    assert st.samples == want["samples"]
    if expect == SPLIT:
        assert st.launches_wavefront == 0 and st.launches_shade > 0 and st.launches_trace > 0, got
    elif expect == FUSED_PART:
        assert st.launches_wavefront > 0 and st.launches_shade > 0 and st.launches_trace > 0, got
    elif expect == FUSED_ALL:
        assert st.launches_wavefront > 0 and st.launches_shade == 0 and st.launches_trace == 0, got
    else:
        assert st.launches_shade > 0 and st.launches_trace > 0, got


@pytest.mark.gpu
def test_gpu_rejects_bad_envmap_descriptors(gpu_ctx, hostmirror, abi):
    """(11) each MSK_ERR_INVALID_ARG case by its message"""
    def fresh(**kw):
        return hostmirror.flatten(plane_meshes(hostmirror), 16, 16, camera=PLANE_CAMERA, env=env_spec(images()["3x5"], **kw))

    def refused(flat, text, envmap=None, plain=False):
        with pytest.raises(abi.MskError) as e:
            if plain:
                h = C.c_void_p()
                gpu_ctx.check(gpu_ctx.lib.msk_gpu_scene_create(gpu_ctx.handle, C.byref(flat.desc), C.byref(h)))
            else:
                abi.Scene(gpu_ctx, flat, envmap=envmap)
        assert text in str(e.value), str(e.value)
        assert e.value.code == abi.MSK_ERR_INVALID_ARG
    abi.Scene(gpu_ctx, fresh()).close()                                # the scene itself is fine
    refused(fresh(), "an envmap emitter needs its image", plain=True)  # a type-2 emitter through plain msk_gpu_scene_create
    plain = hostmirror.flatten(plane_meshes(hostmirror), 16, 16, camera=PLANE_CAMERA, env={"radiance": (0.5, 0.4, 0.3)})
    refused(plain, "the scene has no envmap emitter", envmap=fresh().envmap)
    both = fresh()
    em = (abi.EmitterDesc * 2)(both.desc.emitters[0], abi.EmitterDesc(abi.MSK_EMITTER_CONSTANT, -1, (C.c_float * 3)(0, 0, np.inf), 1e-4, 0))
    both.keep.append(em)
    both.desc.emitters, both.desc.n_emitters = em, 2
    refused(both, "Can only have one environment light")
    em[1].type = abi.MSK_EMITTER_ENVMAP
    refused(both, "Can only have one environment light")
    flat = fresh()
    flat.envmap.width = 0
    refused(flat, "an image of 0 x 5 texels")
    flat = fresh()
    flat.envmap.height = 0
    refused(flat, "an image of 3 x 0 texels")
    for value, text in ((-1.0, "texel 4: the factor w must be finite and non-negative"), (np.inf, "texel 4: the factor w"), (np.nan, "texel 4: the factor w")):
        flat = fresh()
        flat.env_texels.reshape(-1, 4)[4, 3] = value
        refused(flat, text)
    for value in (-1.0, np.inf, np.nan):
        flat = fresh()
        flat.env_weights[7] = value
        refused(flat, "weights must be finite and non-negative")
    flat = fresh()
    flat.env_weights[:] = 0
    refused(flat, "the weights are all zero")
    for m in (np.diag([1, 1, -1]), 2 * np.eye(3), np.array([[1, 0.1, 0], [0, 1, 0], [0, 0, 1]]), np.zeros((3, 3))):
        flat = fresh()
        flat.envmap.to_world[:] = [float(x) for x in m.reshape(-1)]
        refused(flat, "to_world must be a rotation")
    flat = fresh()
    flat.envmap.texels = None
    refused(flat, "texels / weights array missing")
    g = abi.Scene(gpu_ctx, plain)
    with pytest.raises(abi.MskError) as e:
        g.env_sample(np.zeros((1, 2), F))
    assert "the scene has no envmap emitter" in str(e.value)
    g.close()


@pytest.mark.gpu
def test_two_members_behind_one_context(abi, hostmirror):
    """(12) after test_gpu_parity.test_two_members_behind_one_context: a group of two members on device 0 renders the envmap scene;
    the film differs from the single-context film only by the re-association of two partial sums per pixel (that test's criterion),
    and the probes run on the first member.  The developed-image bound of that test is absolute, 1e-4, and the re-association error
    relative (a few 1e-7, times the cancellation of the XYZ to RGB matrix): the scene is lit by the sky alone, at scale 1, so that no
    developed value exceeds 4 (the luminaire's 34 would use up the whole bound)."""
    meshes = [m for m in variant_meshes(hostmirror) if m.name != "cbox_luminaire"]
    flat = hostmirror.flatten(meshes, 48, 48, env=env_spec(lit_image(), skew_rotation(), scale=1.0))
    assert flat.desc.n_emitters == 1
    prm = abi.render_params(spp=9, seed=5)
    with abi.Context(0) as one:
        s1 = abi.Scene(one, flat)
        ref, st1 = s1.render(prm)
        d1 = s1.env_sample(np.array([(0.3, 0.6)], F))
        s1.close()
    with abi.Context((0, 0)) as grp:
        s2 = abi.Scene(grp, flat)
        film, st2 = s2.render(prm)
        serial, _ = s2.render(pcg(abi, spp=2, seed=5))
        d2 = s2.env_sample(np.array([(0.3, 0.6)], F))
        s2.close()
    assert (st2.samples, st2.segments, st2.shadow_rays) == (st1.samples, st1.segments, st1.shadow_rays)
    assert np.allclose(film, ref, rtol=2e-6, atol=1e-6) and film[..., 4].sum(dtype=np.float64) > 0
    a, b = hostmirror.develop(film)[..., :3], hostmirror.develop(ref)[..., :3]
    assert 0 < b.max() < 4.0 and np.abs(a - b).max() < 1e-4
    assert np.isfinite(serial).all() and serial[..., :3].max() > 0
    assert all(np.array_equal(x, y) for x, y in zip(d1, d2))
