"""Randomised parity sweep: random triangle soups (including slivers and near-degenerate triangles), random BSDFs of
every type, one to three area emitters, optional environment, random integrator properties — the GPU film must equal
the oracle's bit for bit on every one.  usage: fuzz_parity.py n_scenes [first_seed [spp [glass [plastic [lens [lights]]]]]]  (glass is
on when its argument is other than 0, plastic when it is given at all, lens and lights when given and other than 0.  glass turns some meshes of every scene into smooth `dielectric`; plastic turns some
into `plastic` / `roughplastic`; lens gives every scene a `thinlens` sensor; lights adds `spot` and `directional` emitters)"""
import importlib, sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__)))); sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np
abi = importlib.import_module("misaki-render_amd.abi"); hm = importlib.import_module("misaki-render_amd.hostmirror")
import oracle_binding


def random_scene(rng, glass=False, seed=0, plastic=False, lens=False, lights=False):
    """glass=True turns some meshes into the smooth `dielectric` (emitters included: glass that emits); what becomes glass is drawn
    from a generator of its own, made from `seed`, so that `rng` is consumed exactly as without it: a seed's scene with
    glass=False is the scene it always was, and with glass=True it is that scene with some BSDFs exchanged.
    plastic=True does the same for `plastic` and `roughplastic`, from another generator of its own: a relative index in [1, 2.6]
    (sometimes exactly 1), `nonlinear`, alpha 10**U(-4, -0.3), an rgb / uniform / checkerboard base, a specular_reflectance that is 0,
    a constant, an rgb or a table, `twosided`, and sometimes a constant-opacity `mask` over it.
    lights=True adds one to three `spot` / `directional` emitters behind the scene's own (a spot anywhere around the scene, aimed into
    it, half-angles from 5 to 120 degrees, sometimes a hard edge; a sun from any direction), lens=True a `thinlens` sensor (an aperture
    that is 0, small or as wide as the scene, focused before, inside or behind it): each from a generator of its own, drawn after
    everything else, so that a seed's scene without the option is the scene it always was."""
    meshes = []
    n_mesh = rng.randint(3, 9)
    n_light = rng.randint(1, 4)
    for i in range(n_mesh):
        faces = []
        for _ in range(rng.randint(1, 12)):
            c = rng.uniform(-1, 1, 3) * 200 + np.array([278, 273, 280])
            size = 10 ** rng.uniform(0.3, 2.5)
            kind = rng.randint(0, 12)
            if kind >= 10:     # axis-aligned quad on a lattice (exact zeros in normals and ray/plane arithmetic)
                c = np.round(c / 50) * 50
                ax = rng.randint(0, 3); ext = np.round(rng.uniform(20, 300, 2) / 10) * 10
                e0 = np.zeros(3); e1_ = np.zeros(3); e0[(ax + 1) % 3] = ext[0]; e1_[(ax + 2) % 3] = ext[1]
                pts = [c, c + e0, c + e0 + e1_, c + e1_]
            elif kind == 0:      # sliver
                a, b = rng.normal(size=3) * size, rng.normal(size=3) * size
                pts = [c, c + a, c + a * (1 + 1e-4) + b * 1e-4]
            elif kind == 1:    # quad
                a, b = rng.normal(size=3) * size, rng.normal(size=3) * size
                pts = [c, c + a, c + a + b, c + b]
            else:
                pts = [c + rng.normal(size=3) * size for _ in range(3)]
            faces.append(tuple(tuple(float(np.float32(v)) for v in p) for p in pts))
        refl = tuple(float(x) for x in rng.uniform(0.05, 0.95, 3))
        t = rng.randint(0, 4)
        bsdf = None
        if t == 1:
            bsdf = {"type": "roughconductor", "alpha": float(10 ** rng.uniform(-2.5, -0.3)), "eta": tuple(rng.uniform(0.1, 3, 3)),
                    "k": tuple(rng.uniform(0.5, 4, 3)), "twosided": bool(rng.randint(0, 2)), "sample_visible": bool(rng.randint(0, 2))}
        elif t == 2:
            bsdf = {"type": "roughdielectric", "alpha": float(rng.choice([0.0, 10 ** rng.uniform(-2.5, -0.3)])), "int_ior": float(rng.uniform(1.05, 2.6)),
                    "ext_ior": float(rng.choice([1.0, 1.33])), "sample_visible": bool(rng.randint(0, 2))}
        elif t == 3:
            bsdf = {"type": "roughconductor", "alpha": (float(rng.uniform(0.02, 0.5)), float(rng.uniform(0.02, 0.5))),
                    "eta": (1.5, 1.5, 1.5), "k": (3.0, 3.0, 3.0), "twosided": True}
        if t == 0:
            # textured reflectance on some diffuse surfaces; drawn from a side stream so that the seed -> geometry mapping of
            # earlier sweeps stays what it was
            trng = np.random.RandomState(int(refl[0] * 1e9) % (2 ** 31))
            if trng.randint(0, 6) == 0:
                refl = float(trng.choice([0.0, 1.0, trng.uniform(0.05, 0.95)]))       # a `uniform` spectrum (spectra/uniform.cpp)
            elif trng.randint(0, 3) == 0:
                m = np.zeros(16)
                m[[0, 1, 2, 4, 5, 6]] = trng.uniform(-12, 12, 6) * (trng.uniform(size=6) < 0.8)
                m[15] = 1
                bsdf = {"type": "diffuse", "twosided": bool(trng.randint(0, 2)),
                        "texture": {"type": "checkerboard", "color0": refl, "color1": tuple(float(x) for x in trng.uniform(0.02, 0.98, 3)),
                                    "matrix": [float(np.float32(x)) for x in m]}}
        rad = tuple(float(x) for x in rng.uniform(1, 30, 3)) if i < n_light else None
        meshes.append(hm.MeshSpec("m%d" % i, faces, refl, radiance=rad, bsdf=bsdf))
    if rng.randint(0, 7) == 0:      # a mesh big enough for the HBM traversal kernels (tree > 48 KB)
        res = int(rng.randint(25, 70))
        blob = hm.blob_mesh("blob", tuple(float(x) for x in rng.uniform(150, 400, 3)), float(rng.uniform(40, 120)), res, res,
                            tuple(float(x) for x in rng.uniform(0.1, 0.9, 3)), seed=int(rng.randint(0, 100)), bump=float(rng.uniform(0, 0.3)))
        if rng.randint(0, 2):
            blob.bsdf = {"type": "roughdielectric", "alpha": 0.1, "int_ior": 1.5, "ext_ior": 1.0}
        meshes.append(blob)
    env = None
    if rng.randint(0, 3) == 0:
        env = {"radiance": tuple(float(x) for x in rng.uniform(0.1, 1.0, 3)) if rng.randint(0, 2) else None, "first": bool(rng.randint(0, 2))}
    camera = None
    if rng.randint(0, 5) == 0:       # the whole scene (and the camera) at another scale: epsilons, clip planes, pdf magnitudes
        sc = float(rng.choice([1e-3, 1e-2, 30.0, 1e3]))
        for m in meshes:
            m.faces = [tuple(tuple(float(np.float32(v * sc)) for v in p) for p in f) for f in m.faces]
        c = hm.CBOX_CAMERA
        camera = dict(fov=float(rng.uniform(20, 90)), near=c["near"] * sc, far=c["far"] * sc, origin=tuple(v * sc for v in c["origin"]),
                      target=tuple(v * sc for v in c["target"]), up=c["up"])
    frng = np.random.RandomState(len(meshes) * 7919 + int(meshes[0].faces[0][0][0] * 1e3) % 100003)    # side stream: filter width
    stddev = float(frng.choice([0.5, 0.5, 0.5, 0.3, 0.625, 0.9]))
    fw, fh = [(48, 40), (48, 40), (33, 17), (64, 64), (7, 5), (100, 3), (1, 1), (37, 53)][frng.randint(0, 8)]      # ragged films, films smaller than a block
    crop = None
    if frng.randint(0, 4) == 0:      # a crop window (film.cpp:12-21): anywhere in the film, down to one pixel (side stream again)
        cw, ch = int(frng.randint(1, fw + 1)), int(frng.randint(1, fh + 1))
        crop = (int(frng.randint(0, fw - cw + 1)), int(frng.randint(0, fh - ch + 1)), cw, ch)
    # tabulated (`regular`) spectra on a quarter of the scenes (ABI v7; side stream): any of a diffuse reflectance, a conductor's
    # eta / k, a dielectric's transmittance, an emitter's radiance, the environment's — tables of 2 … 95 values on grids that
    # cover the sampled wavelengths, start inside them or end inside them (the end segments are then continued)
    trng = np.random.RandomState((len(meshes) * 104729 + int(abs(meshes[0].faces[0][0][1]) * 1e3)) % 1000003)
    if trng.randint(0, 4) == 0:
        def table(lo, hi):
            n = int(trng.choice([2, 3, 5, 16, 31, 48, 95]))
            l0 = float(np.float32(trng.choice([300.0, 360.0, 380.0, 450.0])))
            l1 = float(np.float32(l0 + trng.choice([150.0, 320.0, 470.0, 600.0])))
            return hm.Regular(l0, l1, trng.uniform(lo, hi, n).astype(np.float32))
        for m in meshes:
            if trng.randint(0, 3):
                continue
            if m.bsdf is None and not np.isscalar(m.reflectance):
                m.reflectance = table(0.02, 0.95)
            elif m.bsdf and m.bsdf["type"] == "roughconductor":
                m.bsdf["eta"], m.bsdf["k"] = table(0.1, 3.0), table(0.5, 4.0)
                if trng.randint(0, 2):
                    m.bsdf["specular_reflectance"] = table(0.3, 1.0)
            elif m.bsdf and m.bsdf["type"] == "roughdielectric":
                m.bsdf["specular_transmittance"] = table(0.2, 1.0)
            if m.radiance is not None and trng.randint(0, 2):
                m.radiance = table(0.01, 0.4)
        if env is not None and trng.randint(0, 2):
            env["radiance"] = table(0.001, 0.02)
    if glass:
        grng = np.random.RandomState((int(seed) * 2654435761 + 0x61a55) % (2 ** 32))
        def tint():
            k = grng.randint(0, 5)
            if k == 0:
                return float(grng.uniform(0.2, 1.0))                                   # `uniform`
            if k == 1:
                return hm.Regular(360.0, 830.0, grng.uniform(0.2, 1.0, int(grng.choice([2, 7, 31]))).astype(np.float32))
            if k == 2:
                return tuple(float(x) for x in grng.uniform(0.05, 1.0, 3))             # rgb
            return (1.0, 1.0, 1.0)
        n_glass = 0
        for k, m in enumerate(meshes):
            # every third mesh on average, and at least one per scene (the last one, if none was drawn before it)
            if grng.randint(0, 3) and not (n_glass == 0 and k == len(meshes) - 1):
                continue
            n_glass += 1
            ior = float(grng.uniform(1.05, 2.6))
            inside_dense = bool(grng.randint(0, 2))                                   # either side dense
            m.bsdf = {"type": "dielectric", "int_ior": ior if inside_dense else float(grng.choice([1.0, 1.33])),
                      "ext_ior": float(grng.choice([1.0, 1.33])) if inside_dense else ior,
                      "specular_reflectance": tint(), "specular_transmittance": tint()}
            if isinstance(m.reflectance, hm.Regular) or np.isscalar(m.reflectance):
                m.reflectance = (0.5, 0.5, 0.5)                                        # (unused by the BSDF)
    if plastic:
        prng = np.random.RandomState((int(seed) * 2246822519 + 0x91a571c) % (2 ** 32))
        n_plastic = 0
        for k, m in enumerate(meshes):
            # every third mesh on average, and at least one per scene (the last one, if none was drawn before it)
            if prng.randint(0, 3) and not (n_plastic == 0 and k == len(meshes) - 1):
                continue
            n_plastic += 1
            kind = prng.randint(0, 4)
            if kind == 0:
                base = float(prng.choice([0.0, 1.0, prng.uniform(0.05, 0.95)]))          # `uniform`
            elif kind == 1:
                mat = np.zeros(16)
                mat[[0, 1, 2, 4, 5, 6]] = prng.uniform(-12, 12, 6) * (prng.uniform(size=6) < 0.8)
                mat[15] = 1
                base = {"type": "checkerboard", "color0": tuple(float(x) for x in prng.uniform(0.02, 0.98, 3)), "color1": tuple(float(x) for x in prng.uniform(0.02, 0.98, 3)),
                        "matrix": [float(np.float32(x)) for x in mat]}
            else:
                base = tuple(float(x) for x in prng.uniform(0.05, 0.95, 3))               # rgb
            kind = prng.randint(0, 5)
            if kind == 0:
                coat = 0.0                                                                # no coat at all: ssw = 0
            elif kind == 1:
                coat = float(prng.uniform(0.2, 1.0))
            elif kind == 2:
                coat = hm.Regular(360.0, 830.0, prng.uniform(0.2, 1.0, int(prng.choice([2, 7, 31]))).astype(np.float32))
            else:
                coat = tuple(float(x) for x in prng.uniform(0.05, 1.0, 3))
            spec = {"type": "plastic", "diffuse_reflectance": base, "specular_reflectance": coat, "int_ior": 1.0 if prng.randint(0, 10) == 0 else float(prng.uniform(1.0, 2.6)),
                    "ext_ior": 1.0, "nonlinear": bool(prng.randint(0, 2)), "twosided": bool(prng.randint(0, 2))}
            if prng.randint(0, 2):
                spec.update(type="roughplastic", alpha=float(10 ** prng.uniform(-4, -0.3)))
            m.bsdf = {"type": "mask", "opacity": float(prng.choice([0.25, 0.5, 0.9, 1.0])), "bsdf": spec} if prng.randint(0, 4) == 0 else spec
            if isinstance(m.reflectance, hm.Regular) or np.isscalar(m.reflectance):
                m.reflectance = (0.5, 0.5, 0.5)                                        # (unused by the BSDF)
    unit = (camera["near"] / hm.CBOX_CAMERA["near"]) if camera else 1.0      # the scene's scale against the Cornell box's
    light_specs = []
    if lights:
        lrng = np.random.RandomState((int(seed) * 3266489917 + 0x5907) % (2 ** 32))
        for _ in range(lrng.randint(1, 4)):
            if lrng.randint(0, 3) == 0:
                light_specs.append({"type": "directional", "irradiance": tuple(float(x) for x in lrng.uniform(0.5, 8.0, 3)), "direction": tuple(float(x) for x in lrng.normal(size=3))})
                continue
            origin = (lrng.uniform(-1, 1, 3) * 450 + np.array([278, 273, 280])) * unit
            target = (lrng.uniform(-1, 1, 3) * 150 + np.array([278, 273, 280])) * unit
            cutoff = float(lrng.uniform(5.0, 120.0))
            beam = cutoff if lrng.randint(0, 5) == 0 else float(cutoff * lrng.uniform(0.1, 1.0))
            k = lrng.randint(0, 3)
            inten = float(lrng.uniform(1e4, 1e6)) if k == 0 else tuple(float(x) for x in lrng.uniform(1e4, 1e6, 3))
            inten = tuple(v * unit * unit for v in inten) if isinstance(inten, tuple) else inten * unit * unit
            light_specs.append({"type": "spot", "intensity": inten, "cutoff_angle": cutoff, "beam_width": beam,
                                "lookat": {"origin": tuple(float(v) for v in origin), "target": tuple(float(v) for v in target), "up": (0.0, 1.0, 0.0) if lrng.randint(0, 2) else (0.3, 0.2, 1.0)}})
    flat = hm.flatten(meshes, fw, fh, env=env, camera=camera, filter_stddev=stddev, crop=crop, lights=light_specs)
    if lens:
        arng = np.random.RandomState((int(seed) * 668265263 + 0x1e45) % (2 ** 32))
        radius = float(arng.choice([0.0, 2.0, 25.0, 300.0]) * arng.uniform(0.5, 1.5) * unit)
        focus = float(arng.choice([200.0, 800.0, 1100.0, 4000.0]) * arng.uniform(0.7, 1.3) * unit)
        flat.lens = abi.LensDesc(float(np.float32(radius)), float(np.float32(focus)))
    # vertex normals (perturbed face normals) and texture coordinates on some meshes: mesh.cpp:68-96
    verts, faces = flat.vertices, flat.faces
    for i in range(flat.desc.n_meshes):
        md = flat.desc.meshes[i]
        mode = rng.randint(0, 4)
        if mode == 0 or md.face_count == 0:
            continue
        for f in range(md.first_face, md.first_face + md.face_count):
            idx = md.first_vertex + faces[f]
            p = verts[idx, :3].astype(np.float64)
            n = np.cross(p[1] - p[0], p[2] - p[0])
            ln = np.linalg.norm(n)
            n = n / ln if ln > 0 else np.array([0.0, 0.0, 1.0])
            for k in idx:
                q = n + rng.normal(size=3) * 0.3
                verts[k, 3:6] = (q / np.linalg.norm(q)).astype(np.float32)
                verts[k, 6:8] = rng.uniform(0, 1, 2).astype(np.float32)
        md.has_normals = 1 if mode in (1, 3) else 0
        md.has_texcoords = 1 if mode in (2, 3) else 0
    return flat


def scene_digest(flat):
    """sha256 over everything a flattened scene hands to the back ends (the arrays' contents, not their addresses)"""
    import hashlib
    d = flat.desc
    h = hashlib.sha256()
    h.update(flat.vertices.tobytes()); h.update(flat.faces.tobytes())
    for arr, n in ((d.meshes, d.n_meshes), (d.bsdfs, d.n_bsdfs), (d.emitters, d.n_emitters), (d.textures, d.n_textures), (d.regular_spectra, d.n_regular_spectra)):
        for i in range(n):
            h.update(bytes(arr[i]))
    h.update(np.ctypeslib.as_array(d.regular_values, (max(1, d.n_regular_values),))[:d.n_regular_values].tobytes())
    h.update(bytes(d.camera)); h.update(bytes(d.film))
    return h.hexdigest()


def random_params(rng):
    kw = dict(spp=int(rng.choice([1, 4, 4, 7])), seed=int(rng.randint(0, 1000)), rr_depth=int(rng.choice([1, 2, 5])),
              max_depth=int(rng.choice([-1, -1, 1, 3, 6])), hide_emitters=int(rng.randint(0, 2)), block_size=int(rng.choice([8, 16, 32])))
    if rng.randint(0, 4) == 0:       # a multi-GPU shard of the job (tiles or sample indices)
        world = int(rng.randint(2, 5))
        if rng.randint(0, 2):
            kw.update(block_first=int(rng.randint(0, world)), block_stride=world)
        elif rng.randint(0, 2):
            kw.update(sample_first=int(rng.randint(0, world)), sample_stride=world)
        else:                        # a contiguous sample range [a, spp)
            kw.update(sample_first=int(rng.randint(0, kw["spp"])), sample_stride=1)
    return kw


def sweep(ctx, orc, seeds, verbose=True, spp=None, glass=False, plastic=False, lens=False, lights=False):
    bad = []
    for s in seeds:
        rng = np.random.RandomState(s)
        flat = random_scene(rng, glass=glass, seed=s, plastic=plastic, lens=lens, lights=lights)
        kw = random_params(rng)
        if spp:
            kw["spp"] = spp
        g, o = abi.Scene(ctx, flat), orc.scene(flat)
        film, st = g.render(abi.render_params(**kw))
        ref, rst = o.render(abi.render_params(**kw), threads=8)
        if rng.randint(0, 4) == 0:        # the "aov" integrator on the same scene, random channel list
            types = [int(t) for t in rng.randint(0, 6, rng.randint(1, 5))]
            if types.count(5) > 1:
                types = [t for t in types if t != 5] + [5]
            fa, _ = g.render_aov(abi.render_params(**kw), types)
            ra, _ = o.render_aov(abi.render_params(**kw), types)
            if not np.array_equal(fa.view(np.uint32), ra.view(np.uint32)):
                film = None
        if film is None or not np.array_equal(film.view(np.uint32), ref.view(np.uint32)):
            bad.append(s)
            if verbose:
                print("seed %d differs (%s) params %s" % (s, "aov film" if film is None else "film", kw))
        g.close(); o.close()
    return bad


if __name__ == "__main__":
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 50
    seed0 = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    spp = int(sys.argv[3]) if len(sys.argv) > 3 else None        # optional: samples per pixel for every scene
    on = lambda k: len(sys.argv) > k and sys.argv[k] != "0"
    bad = sweep(abi.Context(0), oracle_binding.load(), range(seed0, seed0 + n), spp=spp or None, glass=on(4), plastic=len(sys.argv) > 5, lens=on(6), lights=on(7))
    print("fuzz: %d scenes, %d with a film different from the oracle's" % (n, len(bad)))
    sys.exit(1 if bad else 0)
