// msk_serial_body.inc — the body of k_path_serial / k_path_serial_d / k_path_serial_b / k_path_serial_e / k_path_serial_p / k_path_serial_m (msk_serial.h), included once into each: `TB` is the
// kernel's table type, `sc` and `prm` its arguments.  Written once and stamped, not shared through a function, so that
// k_path_serial compiles from the token stream it always had.
    extern __shared__ float4 lds_dyn[];
    uint32_t *stack_base = (uint32_t *) lds_dyn;
    const LaneStack<true> stack{stack_base + threadIdx.x, prm.stack_ovf + (size_t) blockIdx.x * MSK_BLOCK + threadIdx.x,
                                (int) sc.stack_entries, (size_t) gridDim.x * MSK_BLOCK, nullptr};
    // one image block per lane — or, while there are fewer blocks than the GPU has room for waves, per WAVE (lane 0): 64 scalar
    // loops packed into one wave execute the union of their branches, one loop per wave executes its own (prm.per_wave)
    const uint32_t tid = blockIdx.x * MSK_BLOCK + threadIdx.x;
    if (prm.per_wave && (threadIdx.x & (MSK_WAVE - 1u))) return;
    const uint32_t bi = prm.per_wave ? tid / MSK_WAVE : tid;
    if (bi >= prm.n_blocks) return;
    TB tb;                                  // (the fidelity mode carries the table forms of tabulated spectra always: one instantiation)
    static_cast<SceneTables &>(tb) = stage_tables<false>(sc, nullptr);
    const BlockInfo b = prm.blocks[bi];
    const int border = sc.filter_border;
    const int sx = b.size_x + 2 * border, sy = b.size_y + 2 * border;
    float *data = prm.block_buf + (size_t) b.slot * prm.buf_stride;
    Pcg32 rng;
    rng.seed(0x853c49e6748fea9bULL + prm.seed, 0xda3e39cb94b95bdbULL);      // oracle D2; independent.cpp:20-26
    const uint32_t n_em = sc.n_emitters;
    const uint32_t sstride = prm.sample_stride ? prm.sample_stride : 1u;
    unsigned long long n_samples = 0, n_segments = 0, n_shadow = 0, n_invalid = 0;
    auto closest = [&](f3 o, f3 d, float tmin, float tmax) {
        float t, u, v; uint32_t prim;
        traverse<false, true>(sc.nodes, sc.tris, sc.tri_pad, sc.root_ref, sc.n_tris, o, d, tmin, tmax, stack, &t, &u, &v, &prim);
        const bool valid = (prim != MSK_NO_PRIM) && (t != tmax);                // scene.cpp:234
        return make_float4(valid ? t : MSK_INF_F, u, v, __uint_as_float(valid ? (prim & MSK_PRIM_ID) : MSK_PRIM_ID));
    };
    for (int y = 0; y < b.size_y; ++y)
        for (int x = 0; x < b.size_x; ++x)
            for (uint32_t s = 0; s < prm.spp; ++s) {
                if (s < prm.sample_first || (s - prm.sample_first) % sstride != 0u) continue;      // msk_gpu.h: s = first + k stride
                // ---- render_sample (integrator.cpp:103-126)
                const float jx = rng.next_float(), jy = rng.next_float();
                const float wsample = rng.next_float();
                (void) rng.next_float(); (void) rng.next_float();                   // the aperture sample (perspective.cpp:22: unused)
                const float px = (float) (x + b.off_x) + jx, py = (float) (y + b.off_y) + jy;
                spec wl;
#pragma unroll
                for (int q = 0; q < 4; ++q) wl.v[q] = wavelength_of(wsample, q);
                float r4[4];
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    r4[q] = ((sc.s2c[q * 4 + 0] * px + sc.s2c[q * 4 + 1] * py) + sc.s2c[q * 4 + 2] * 0.f) + sc.s2c[q * 4 + 3] * 1.f;
                const f3 near_p = mk3(r4[0] / r4[3], r4[1] / r4[3], r4[2] / r4[3]);
                const f3 dl = normalized(near_p);
                const float inv_z = 1.f / dl.z;
                float o4[4];
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    o4[q] = ((sc.to_world[q * 4 + 0] * 0.f + sc.to_world[q * 4 + 1] * 0.f) + sc.to_world[q * 4 + 2] * 0.f) + sc.to_world[q * 4 + 3] * 1.f;
                f3 ro = mk3(o4[0] / o4[3], o4[1] / o4[3], o4[2] / o4[3]);
                const float *m = sc.to_world;
                f3 rd = mk3(m[0] * dl.x + (m[1] * dl.y + m[2] * dl.z), m[4] * dl.x + (m[5] * dl.y + m[6] * dl.z), m[8] * dl.x + (m[9] * dl.y + m[10] * dl.z));
                ++n_samples;
                // ---- PathTracer::sample (path.cpp:23-125), the scalar loop
                spec thr = splat(1.f), res = splat(0.f);
                float eta = 1.f;
                bool scattered = false;                                                // path.cpp:31,73 (read only where tb_traits<TB>::mask)
                ++n_segments;
                float4 hit = closest(ro, rd, sc.near_clip * inv_z, sc.far_clip * inv_z);
                for (int depth = 1; depth <= prm.max_depth || prm.max_depth < 0; ++depth) {
                    if (hit.x == MSK_INF_F) {                                          // path.cpp:34-41
                        if (tb_traits<TB>::envmap && (!tb_traits<TB>::delta || env_is_image(tb, sc))) {
                            if (depth == 1 && !prm.hide_emitters) { const EnvView ev = env_view(tb, sc.env_emitter); float sin_t; const f2 uv = env_dir_to_uv(ev, rd, &sin_t); res = res + thr * env_radiance(ev, tb, sc.env_emitter, uv, wl); }
                        } else
                        if (depth == 1 && !prm.hide_emitters && sc.env_emitter >= 0) res = res + thr * emitter_radiance(tb, sc.env_emitter, wl);
                        break;
                    }
                    const Interaction si = make_interaction(tb, hit, rd);
                    BsdfRec bs = load_bsdf(tb, si.bsdf_id);
                    f3 wi_s = si.wi;
                    bool flipped = false;
                    {
                        const int back = __float_as_int(bs.a.y);
                        if (back >= 0 && wi_s.z < 0.f) { wi_s.z = -wi_s.z; flipped = true; if (back != si.bsdf_id) bs = load_bsdf(tb, back); }
                    }
                    if (si.emitter_id >= 0 && depth == 1 && !prm.hide_emitters && si.wi.z > 0.f)      // path.cpp:42-47, area.cpp:51-54
                        res = res + thr * emitter_radiance(tb, si.emitter_id, wl);
                    if (depth >= prm.max_depth && prm.max_depth > 0) break;             // path.cpp:48-49
                    spec refl = splat(0.f);
                    if (__float_as_int(bs.a.x) == 0 || (tb_traits<TB>::mask && (__float_as_int(bs.a.x) == MSK_BSDF_PLASTIC || __float_as_int(bs.a.x) == MSK_BSDF_ROUGHPLASTIC))) {      // (a plastic's base as the diffuse BSDF)
                        const uint32_t tex = __float_as_uint(bs.ior.z);
                        refl = reflectance_eval(tb, mk3(bs.a.z, bs.a.w, bs.b.x), bs.ior.w, tex, [&]() { return hit_uv(tb, hit); }, wl);
                    }
                    float opacity = 1.f;                                               // of the entry the mesh names (msk_gpu.h, msk_mask_desc)
                    if (tb_traits<TB>::mask) opacity = mask_opacity(tb, mask_record(sc, si.bsdf_id), [&]() { return hit_uv(tb, hit); });
                    const float tmin = (1.f + max_abs(si.p)) * MSK_RAY_EPS_F;          // interaction.h:40-44
                    // ---- next-event estimation (path.cpp:56-67, scene.cpp:68-103); the draw is made whatever the scene holds —
                    // but not at a BSDF without a smooth lobe (a `dielectric`), where path.cpp:56 skips the sample and its next2d()
                    float nee_pdf = 0.f;
                    const bool delta = bsdf_is_delta<TB>(bs);
                    if (!delta) {
                        f2 u; u.x = rng.next_float(); u.y = rng.next_float();
                        if (n_em > 0) {
                            uint32_t e = 0;
                            float light_sel_pdf = 1.f;
                            if (n_em > 1) {
                                light_sel_pdf = 1.f / n_em;
                                uint32_t index = (uint32_t) (u.x * (float) n_em);
                                index = index < n_em - 1 ? index : n_em - 1;
                                u.x = (u.x - index * light_sel_pdf) * n_em;
                                e = index;
                            }
                            const float4 e0 = tb.emitters[2 * e], e1 = tb.emitters[2 * e + 1];
                            f3 d; float dist, pdf; spec emitter_val;
                            bool point = false;
                            if (tb_traits<TB>::delta && emitter_is_delta(__float_as_uint(e1.x))) {   // point.cpp (msk_gpu.h, msk_point_desc); spot, sun (msk_light_desc)
                                f3 k;
                                d = delta_light_sample(tb, sc, __float_as_uint(e1.x), e0, e1, si.p, &dist, &k, &pdf);
                                point = true;
                                emitter_val = emitter_radiance(tb, (int) e, wl) * k.x * k.y * k.z;
                                if (pdf == 0.f) emitter_val = splat(0.f);
                            } else
                            if (tb_traits<TB>::envmap && (int) e == sc.env_emitter && (!tb_traits<TB>::delta || env_is_image(tb, sc))) {  // the image (msk_gpu.h, msk_envmap_desc)
                                const EnvView ev = env_view(tb, (int) e);
                                f2 uv;
                                d = env_sample(ev, u, &uv, &pdf);
                                dist = 2.f * sc.env_radius;
                                emitter_val = splat(0.f);
                                if (pdf != 0.f) emitter_val = env_radiance(ev, tb, (int) e, uv, wl) / pdf;
                                nee_pdf = pdf;
                            } else
                            if ((int) e == sc.env_emitter) {                           // constant.cpp:53-72
                                d = square_to_uniform_sphere(u);
                                dist = 2.f * sc.env_radius;
                                pdf = MSK_INV_FOUR_PI_F;
                                emitter_val = emitter_radiance(tb, (int) e, wl) / pdf;
                                nee_pdf = pdf;
                            } else {
                                const uint32_t first_face = __float_as_uint(e1.y), n_faces = __float_as_uint(e1.z);
                                const float *cdf = tb.cdf + __float_as_uint(e1.w);
                                uint32_t lo = 0, hi = n_faces + 1;                     // Distribution1D::sample_reuse (core/distribution.h:106-116)
                                while (lo < hi) { uint32_t mid = (lo + hi) >> 1; if (!(u.y < cdf[mid])) lo = mid + 1; else hi = mid; }
                                int fidx = (int) lo - 1;
                                fidx = fidx < 0 ? 0 : fidx; fidx = fidx > (int) n_faces - 1 ? (int) n_faces - 1 : fidx;
                                u.y = (u.y - cdf[fidx]) / (cdf[fidx + 1] - cdf[fidx]);
                                const uint32_t lprim = first_face + (uint32_t) fidx;
                                const float4 la = tb.tri_verts[(size_t) lprim * 3], lb = tb.tri_verts[(size_t) lprim * 3 + 1], lc = tb.tri_verts[(size_t) lprim * 3 + 2];
                                const f3 p0 = mk3(la.x, la.y, la.z), p1 = mk3(lb.x, lb.y, lb.z), p2 = mk3(lc.x, lc.y, lc.z);
                                const f3 ed0 = p1 - p0, ed1 = p2 - p0;                 // mesh.cpp:103-133
                                const f2 bc = square_to_uniform_triangle(u);
                                const f3 lp = p0 + ed0 * bc.x + ed1 * bc.y;
                                const float4 lf = tb.tri_frames[(size_t) lprim * 3];
                                f3 ln = mk3(lf.x, lf.y, lf.z);
                                const int4 lmi = tb.mesh_info[__float_as_uint(la.w)];
                                if (lmi.z & 1) {
                                    const float4 na = tb.tri_normals[(size_t) lprim * 3], nb = tb.tri_normals[(size_t) lprim * 3 + 1], nc = tb.tri_normals[(size_t) lprim * 3 + 2];
                                    ln = normalized(mk3(na.x, na.y, na.z) * (1.f - bc.x - bc.y) + mk3(nb.x, nb.y, nb.z) * bc.x + mk3(nc.x, nc.y, nc.z) * bc.y);
                                }
                                pdf = e0.w;
                                d = lp - si.p;                                         // shape.cpp:64-78
                                const float dist2 = dot(d, d);
                                dist = __builtin_sqrtf(dist2);
                                d = d / dist;
                                const float dp = fabsf(dot(d, ln));
                                pdf *= (dp != 0.f) ? dist2 / dp : 0.f;
                                nee_pdf = e0.w * ((dp != 0.f) ? (dist * dist) / dp : 0.f);   // shape.cpp:80-86
                                if (dot(d, ln) < 0.f && pdf != 0.f) emitter_val = emitter_radiance(tb, (int) e, wl) / pdf;   // area.cpp:39-44
                                else { pdf = 0.f; emitter_val = splat(0.f); }
                            }
                            if (n_em > 1) { pdf *= light_sel_pdf; emitter_val = emitter_val * (float) n_em; nee_pdf = nee_pdf * (1.f / n_em); }
                            if (pdf != 0.f) {
                                f3 wo = si.sh.to_local(d);
                                if (flipped) wo.z = -wo.z;
                                spec bsdf_val; float bsdf_pdf;
                                bsdf_eval_pdf<false>(tb, bs, wi_s, wo, wl, refl, &bsdf_val, &bsdf_pdf);
                                if (tb_traits<TB>::mask) { bsdf_val = bsdf_val * opacity; bsdf_pdf = opacity * bsdf_pdf; }
                                const float w = (tb_traits<TB>::delta && point) ? 1.f : mis_weight(pdf, bsdf_pdf);     // a delta light: weight 1
                                const spec contrib = thr * emitter_val * bsdf_val * w;
                                if (any_nonzero(contrib)) {                            // scene.cpp:91-95: an occluded sample adds nothing
                                    ++n_shadow;
                                    float t, uu, vv; uint32_t pp_;
                                    const bool occluded = traverse<true, true>(sc.nodes, sc.tris, sc.tri_pad, sc.root_ref, sc.n_tris, si.p, d, tmin,
                                                                               dist * (1.f - MSK_SHADOW_EPS_F), stack, &t, &uu, &vv, &pp_);
                                    if (!occluded) res = res + contrib;
                                }
                            }
                        }
                    }
                    // ---- BSDF sampling (path.cpp:71-80)
                    const float sample1 = rng.next_float();
                    f2 u2; u2.x = rng.next_float(); u2.y = rng.next_float();
                    f3 wo_l; bool ok; float bs_pdf, bs_eta;
                    // a mask picks its lobe by u.x (mask.cpp:43-44): the nested BSDF with u.x / a, or the null lobe along the ray's own direction
                    const bool null_lobe = tb_traits<TB>::mask && !mask_pick_nested(opacity, &u2);
                    spec bsdf_val;
                    bool coat = false;                                                 // a plastic sampled its delta coat (set only where tb_traits<TB>::mask)
                    if (tb_traits<TB>::mask && null_lobe) { bsdf_val = splat(1.f); bs_pdf = 1.f - opacity; bs_eta = 1.f; ok = true; wo_l = mk3(0.f, 0.f, 0.f); }
                    else if constexpr (tb_traits<TB>::mask) {
                        bsdf_val = bsdf_sample<false>(tb, bs, wi_s, sample1, u2, wl, refl, &wo_l, &bs_pdf, &bs_eta, &ok, &coat);
                        bs_pdf = opacity * bs_pdf; scattered = true;
                    } else {
                        bsdf_val = bsdf_sample<false>(tb, bs, wi_s, sample1, u2, wl, refl, &wo_l, &bs_pdf, &bs_eta, &ok);
                    }
                    const bool hidden = tb_traits<TB>::mask && prm.hide_emitters && !scattered;      // path.cpp:92-93; DESIGN.md section 9, departure 8
                    f3 wo = mk3(0.f, 0.f, 0.f);
                    if (ok) { if (flipped) wo_l.z = -wo_l.z; wo = si.sh.to_world(wo_l); if (tb_traits<TB>::mask && null_lobe) wo = rd; ++n_segments; }
                    // the sampled ray (a failed sample's zero direction finds nothing: path.cpp:89-97)
                    ro = si.p; rd = wo;
                    const float4 hit_b = ok ? closest(ro, rd, tmin, MSK_INF_F) : make_float4(MSK_INF_F, 0.f, 0.f, __uint_as_float(MSK_PRIM_ID));
                    spec value = splat(0.f);
                    bool hit_emitter = false;
                    float emitter_pdf = 0.f;
                    if (hit_b.x != MSK_INF_F) {
                        const Interaction sb = make_interaction(tb, hit_b, rd);
                        if (sb.emitter_id >= 0) {                                      // path.cpp:82-88; records.cpp:7-14; scene.cpp:105-112
                            if (sb.wi.z > 0.f) value = emitter_radiance(tb, sb.emitter_id, wl);
                            float pdf = tb.emitters[2 * sb.emitter_id].w;
                            const float dp = fabsf(dot(rd, sb.sh.n));
                            pdf *= (dp != 0.f) ? (sb.t * sb.t) / dp : 0.f;
                            if (n_em != 1) pdf = pdf * (1.f / n_em);
                            emitter_pdf = pdf;
                            hit_emitter = true;
                        }
                    } else if (tb_traits<TB>::envmap && (!tb_traits<TB>::delta || env_is_image(tb, sc))) {                                  // value and density of the ray's own direction
                        const EnvView ev = env_view(tb, sc.env_emitter);
                        float sin_t;
                        const f2 uv = env_dir_to_uv(ev, rd, &sin_t);
                        value = env_radiance(ev, tb, sc.env_emitter, uv, wl);
                        emitter_pdf = env_pdf(ev, uv, sin_t);
                        if (n_em != 1) emitter_pdf = emitter_pdf * (1.f / n_em);
                        hit_emitter = true;
                    } else if (tb_traits<TB>::delta && sc.env_emitter >= 0) {           // the `constant` sky beside a delta light: its own density
                        value = emitter_radiance(tb, sc.env_emitter, wl);
                        emitter_pdf = MSK_INV_FOUR_PI_F;
                        if (n_em != 1) emitter_pdf = emitter_pdf * (1.f / n_em);
                        hit_emitter = true;
                    } else if (sc.env_emitter >= 0) {                                   // path.cpp:90-95: `ds` is the NEE sample's record
                        value = emitter_radiance(tb, sc.env_emitter, wl);
                        emitter_pdf = nee_pdf;
                        hit_emitter = true;
                    } else {
                        break;                                                         // path.cpp:96-97
                    }
                    thr = thr * bsdf_val;                                              // path.cpp:99 (a failed sample: weight 0, pdf 0, eta 1)
                    eta *= bs_eta;                                                     // path.cpp:100
                    if (delta || (tb_traits<TB>::mask && (null_lobe || coat))) emitter_pdf = 0.f;                                      // path.cpp:104-106: BSDFFlags::Delta
                    if (hit_emitter && !hidden) res = res + thr * value * mis_weight(bs_pdf, emitter_pdf);
                    hit = hit_b;
                    if (depth + 1 >= prm.rr_depth) {                                   // path.cpp:116-122
                        const float q = fmin_std(max4(thr) * eta * eta, 0.95f);
                        if (rng.next_float() >= q) break;
                        thr = thr / q;
                    }
                }
                // ---- integrator.cpp:115-125: ray weight, XYZ, splat
                spec wgt;
#pragma unroll
                for (int k = 0; k < 4; ++k) wgt.v[k] = wavelength_weight(wl.v[k]);
                const spec result = res * wgt;
                float v5[5];
                spectrum_to_xyz(tb.cie, result, wl, &v5[0], &v5[1], &v5[2]);
                v5[3] = 1.f; v5[4] = 1.f;
                if (invalid_value(v5[0], v5[1], v5[2], true)) n_invalid += 1;                    // imageblock.cpp:57-81: warned about, splatted all the same
                serial_put(sc, data, sx, sy, b.off_x - border, b.off_y - border, px, py, v5);
            }
    atomicAdd(&prm.counters[0], n_samples); atomicAdd(&prm.counters[1], n_segments); atomicAdd(&prm.counters[2], n_shadow);
    if (n_invalid) atomicAdd(&prm.counters[3], n_invalid);
