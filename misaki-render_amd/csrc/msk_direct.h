// msk_direct.h — the "direct" integrator on the device (included by msk_gpu.hip): integrators/direct.cpp with the semantics
// include/msk_gpu.h pins (msk_direct_params) and DESIGN.md section 9 explains.
//
// A camera sample has a fixed, small ray budget — the primary ray, N = light_samples shadow rays, M = bsdf_samples BSDF rays —
// so there is no path state in HBM, no pool and no wavefront loop: ONE LANE owns ONE SAMPLE through all its rays and writes the
// sample's record, which the film replay of the wavefront path (k_resolve_*, k_film_put) then consumes unchanged.  A wave owns a
// contiguous range of the pass's records (record r = pass pixel r / spp_owned, owned sample r % spp_owned).  Its loop has two
// phases:
//   fill     lanes WITHOUT a primary hit draw the next samples of the wave's range (ballot + prefix count, the project's usual
//            regeneration) and trace their camera rays; a miss is finished where it is found (environment radiance, record) and
//            the lane draws again — until every lane holds a hit or the range is empty;
//   shade    only then the N + M secondary loop runs, with every lane occupied, and the lanes' records are written together.
// A sample's arithmetic is its own and its record is addressed by (pixel, sample): which lane ran it changes nothing.
// The arithmetic of a hit is shade_region's / k_path_serial's, call for call (make_interaction, bsdf_eval_pdf, bsdf_sample, the
// emitter sampling of scene.cpp:68-103, env_*, point_sample), with one table type for every scene: SceneTablesP, the widest.
// MODE: the tree a launch walks (mskplan::DirectPlan::form) — 0 the binary tree staged in LDS, 6 the half-float 4-wide tree in
// HBM, 1 the binary tree in HBM (every other trace mode: any tree gives the same hits).
#pragma once

namespace msk {

struct DirectArgs {
    uint32_t n_light, n_bsdf;                   // N, M
    unsigned long long rec_first, rec_count;    // the records of this launch
    uint32_t per_wave;                          // records a wave owns (a multiple of MSK_WAVE)
    uint32_t tables_mode;                       // 0: tables from HBM / L2, 1: the small ones staged, 2: all staged (DirectPlan)
    uint32_t stack_f4;                          // float4 offset of the traversal stacks in LDS
    uint32_t *stack_ovf;                        // LaneStack overflow, or nullptr
    unsigned long long *counters;               // MSK_DIRECT_COUNTER_LINES x 8: {samples, segments, shadow rays, invalid samples, -}
};
// the counters are spread over this many 64-byte lines (wave index modulo): one hot line of atomics serialises
#define MSK_DIRECT_COUNTER_LINES 64u

// value of a wave-uniform quantity computed inside a divergent branch by the lanes of `mask` (0 when no lane was in it)
MSK_DEV uint32_t direct_from_lanes(uint32_t v, unsigned long long mask) {
    return mask ? (uint32_t) __shfl((int) v, (int) __builtin_ctzll(mask)) : 0u;
}
// the power heuristic over sample counts (msk_gpu.h): (na pa)^2 / ((na pa)^2 + (nb pb)^2), 0 when pa is 0.  With na = nb = 1 the
// products are exact and this is mis_weight(pa, pb), bit for bit.
MSK_DEV float direct_weight(float na, float pa, float nb, float pb) {
    float a = na * pa, b = nb * pb;
    a *= a; b *= b;
    return a > 0.f ? a / (a + b) : 0.f;
}

// Registers: the kernel carries a hit's shading state around three inlined traversals.  Left alone the allocator takes 256 VGPRs
// + 4 AGPRs = one wave per SIMD; held at three waves it fits 164 (MODE 0) / 168 (MODE 6) without scratch, at four it spills
// 84 / 92 bytes per lane (EXPERIMENTS.md): three.
#ifndef MSK_DIRECT_WAVES
#define MSK_DIRECT_WAVES 3, 3
#endif
// LENS: the scene's sensor is a `thinlens` (msk_gpu.h: msk_lens_desc): the camera ray starts on the lens, from pair 2 of the key
template <int MODE, bool LENS = false>
__global__ void __launch_bounds__(MSK_BLOCK) __attribute__((amdgpu_waves_per_eu(MSK_DIRECT_WAVES)))
k_direct(DeviceScene sc, PathState st_unused, PassParams pp, DirectArgs da) {       // (the argument layout emit_record reads: MSK_COLD_KARGS)
    typedef SceneTablesP TB;
    extern __shared__ float4 lds_dyn[];
    // LDS: [staged tables][traversal stacks (+ four words per lane for the trees in HBM)][tree + triangles (MODE 0)]
    TB tb;
    if (da.tables_mode == 2u) static_cast<SceneTables &>(tb) = stage_tables<true>(sc, lds_dyn);
    else static_cast<SceneTables &>(tb) = stage_tables<false>(sc, da.tables_mode ? lds_dyn : nullptr);
    uint32_t *stack_base = (uint32_t *) (lds_dyn + da.stack_f4);
    float4 *scene_lds = lds_dyn + da.stack_f4 + (sc.stack_entries * MSK_BLOCK) / 4;
    const TraceLds g = stage_scene(sc, scene_lds, MODE == 0, false);
    const LaneStack<MSK_OVF(MODE)> stack{stack_base + threadIdx.x, da.stack_ovf + (size_t) blockIdx.x * MSK_BLOCK + threadIdx.x,
                                         (int) sc.stack_entries, (size_t) gridDim.x * MSK_BLOCK,
                                         MSK_OVF(MODE) ? stack_base + sc.stack_entries * MSK_BLOCK + threadIdx.x * 4 : nullptr};
    const uint32_t gwave = (blockIdx.x * MSK_BLOCK + threadIdx.x) / MSK_WAVE;
    const uint32_t lane = threadIdx.x & (MSK_WAVE - 1);
    const unsigned long long below = (1ull << lane) - 1ull;
    unsigned long long next = (unsigned long long) gwave * da.per_wave;               // within the launch
    if (next >= da.rec_count) return;
    const unsigned long long end = next + da.per_wave < da.rec_count ? next + da.per_wave : da.rec_count;
    const uint32_t N = da.n_light, M = da.n_bsdf;
    const float fN = (float) N, fM = (float) M;
    const uint32_t n_em = sc.n_emitters;
    const bool env_image = env_is_image(tb, sc);
    uint32_t n_segments = 0, n_shadow = 0;                                            // this lane's own rays
    uint32_t n_invalid = 0;                                                           // wave-uniform

    auto closest = [&](f3 o, f3 d, float tmin, float tmax) {
        float t, u, v; uint32_t prim;
        traverse_scene<MODE, false>(sc, g, o, d, tmin, tmax, stack, &t, &u, &v, &prim);
        const bool valid = (prim != MSK_NO_PRIM) && (t != tmax);                      // scene.cpp:234
        return make_float4(valid ? t : MSK_INF_F, u, v, __uint_as_float(valid ? (prim & MSK_PRIM_ID) : MSK_PRIM_ID));
    };

    // what a lane holds of its sample between the phases
    bool have = false;
    uint32_t pix = 0, si = 0;
    spec wl = splat(0.f);
    f3 rd = mk3(0.f, 0.f, 0.f);
    float4 hit = make_float4(MSK_INF_F, 0.f, 0.f, 0.f);

    for (;;) {
        // ---- fill: lanes without a primary hit take the next samples of the range, in order
        for (;;) {
            const unsigned long long m_need = __ballot(!have);
            if (m_need == 0ull || next >= end) break;
            const unsigned long long left = end - next;
            const uint32_t rank = (uint32_t) __popcll(m_need & below);
            const bool take = !have && rank < left;
            const uint32_t n_take = (uint32_t) (left < (unsigned long long) __popcll(m_need) ? left : (unsigned long long) __popcll(m_need));
            bool miss = false;
            spec res = splat(0.f);
            if (take) {
                const unsigned long long r = da.rec_first + next + rank;
                const uint32_t j = (r >> 32) ? (uint32_t) (r / pp.spp_owned) : (uint32_t) r / pp.spp_owned;      // (a pass of < 2^32 records: a 32-bit division)
                si = (uint32_t) (r - (unsigned long long) j * pp.spp_owned);
                const uint4 pt = pp.pix_table[j];
                pix = pt.x;
                // ---- render_sample (integrator.cpp:103-116), as shade_region's regeneration
                const uint64_t key = counter_key(pp.seed, pix, pp.sample_first + si * pp.sample_stride);
                const f2 jit = counter_pair(key, 0);
                const float wsample = counter_pair(key, 1).x;
                const float px = (float) pixel_x(sc.filter_border, pt) + jit.x, py = (float) pixel_y(sc.filter_border, pt) + jit.y;
                f2 ap; ap.x = 0.f; ap.y = 0.f;
                if (LENS) ap = counter_pair(key, 2);
                const CameraRay cr = camera_ray<LENS>(sc.s2c, sc.to_world, sc.near_clip, sc.far_clip, sc.lens_radius, sc.focus_distance, px, py, ap);   // msk_lens.h
                const f3 ro = cr.o;
                rd = cr.d;
#pragma unroll
                for (int q = 0; q < 4; ++q) { wl.v[q] = wavelength_of(wsample, q); __builtin_amdgcn_sched_barrier(0); }
                hit = closest(ro, rd, cr.tnear, cr.tfar);
                have = hit.x != MSK_INF_F;
                miss = !have;
                if (miss && !pp.hide_emitters && sc.env_emitter >= 0) {               // path.cpp:34-41
                    if (env_image) {
                        const EnvView ev = env_view(tb, sc.env_emitter);
                        float sin_t;
                        const f2 uv = env_dir_to_uv(ev, rd, &sin_t);
                        res = res + env_radiance(ev, tb, sc.env_emitter, uv, wl);
                    } else res = res + emitter_radiance(tb, sc.env_emitter, wl);
                }
            }
            // a miss is finished here: its record, and the lane draws again
            const unsigned long long m_miss = __ballot(miss);
            uint32_t inv = 0;
            if (miss) inv = emit_record<false>(sc, tb, pp, wl, res, pix, si);
            n_invalid += direct_from_lanes(inv, m_miss);
            if (take) n_segments += 1u;
            next += n_take;
        }
        const unsigned long long m_have = __ballot(have);
        if (m_have == 0ull) break;

        // ---- shade: the primary hit's emission, N light samples, M BSDF samples (in this order)
        uint32_t inv = 0;
        if (have) {
            spec res = splat(0.f);
            const uint64_t key = counter_key(pp.seed, pix, pp.sample_first + si * pp.sample_stride);
            const Interaction is = make_interaction(tb, hit, rd);
            // (the BSDF record — 28 registers — is read again by every secondary sample instead of being carried across its traversal)
            int bsdf_id = is.bsdf_id;
            f3 wi_s = is.wi;
            bool flipped = false;
            bool delta;
            spec refl = splat(0.f);
            {
                BsdfRec bs = load_bsdf(tb, bsdf_id);
                const int back = __float_as_int(bs.a.y);                              // twosided.cpp:38-101
                if (back >= 0 && wi_s.z < 0.f) { wi_s.z = -wi_s.z; flipped = true; if (back != bsdf_id) { bsdf_id = back; bs = load_bsdf(tb, back); } }
                if (__float_as_int(bs.a.x) == 0) {
                    const uint32_t tex = __float_as_uint(bs.ior.z);
                    refl = reflectance_eval(tb, mk3(bs.a.z, bs.a.w, bs.b.x), bs.ior.w, tex, [&]() { return hit_uv(tb, hit); }, wl);
                }
                delta = bsdf_is_delta<TB>(bs);
            }
            if (is.emitter_id >= 0 && !pp.hide_emitters && is.wi.z > 0.f)             // path.cpp:42-47, area.cpp:51-54
                res = res + emitter_radiance(tb, is.emitter_id, wl);
            const float tmin = (1.f + max_abs(is.p)) * MSK_RAY_EPS_F;                 // interaction.h:40-44
            // ---- light samples (path.cpp:56-67, scene.cpp:68-103): not at a BSDF without a smooth lobe
            if (!delta && n_em > 0)
            for (uint32_t i = 0; i < N; ++i) {
                f2 u = counter_pair(key, 3u + i);
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
                if (emitter_is_delta(__float_as_uint(e1.x))) {                        // point.cpp (msk_gpu.h, msk_point_desc); spot, sun (msk_light_desc)
                    f3 k;
                    d = delta_light_sample(tb, sc, __float_as_uint(e1.x), e0, e1, is.p, &dist, &k, &pdf);
                    point = true;
                    emitter_val = emitter_radiance(tb, (int) e, wl) * k.x * k.y * k.z;
                    if (pdf == 0.f) emitter_val = splat(0.f);
                } else
                if ((int) e == sc.env_emitter && env_image) {                         // the image (msk_gpu.h, msk_envmap_desc)
                    const EnvView ev = env_view(tb, (int) e);
                    f2 uv;
                    d = env_sample(ev, u, &uv, &pdf);
                    dist = 2.f * sc.env_radius;
                    emitter_val = splat(0.f);
                    if (pdf != 0.f) emitter_val = env_radiance(ev, tb, (int) e, uv, wl) / pdf;
                } else
                if ((int) e == sc.env_emitter) {                                      // constant.cpp:53-72
                    d = square_to_uniform_sphere(u);
                    dist = 2.f * sc.env_radius;
                    pdf = MSK_INV_FOUR_PI_F;
                    emitter_val = emitter_radiance(tb, (int) e, wl) / pdf;
                } else {
                    const uint32_t first_face = __float_as_uint(e1.y), n_faces = __float_as_uint(e1.z);
                    const float *cdf = tb.cdf + __float_as_uint(e1.w);
                    uint32_t lo = 0, hi = n_faces + 1;                                // Distribution1D::sample_reuse (core/distribution.h:106-116)
                    while (lo < hi) { uint32_t mid = (lo + hi) >> 1; if (!(u.y < cdf[mid])) lo = mid + 1; else hi = mid; }
                    int fidx = (int) lo - 1;
                    fidx = fidx < 0 ? 0 : fidx; fidx = fidx > (int) n_faces - 1 ? (int) n_faces - 1 : fidx;
                    u.y = (u.y - cdf[fidx]) / (cdf[fidx + 1] - cdf[fidx]);
                    const uint32_t lprim = first_face + (uint32_t) fidx;
                    const float4 la = tb.tri_verts[(size_t) lprim * 3], lb = tb.tri_verts[(size_t) lprim * 3 + 1], lc = tb.tri_verts[(size_t) lprim * 3 + 2];
                    const f3 p0 = mk3(la.x, la.y, la.z), p1 = mk3(lb.x, lb.y, lb.z), p2 = mk3(lc.x, lc.y, lc.z);
                    const f3 ed0 = p1 - p0, ed1 = p2 - p0;                            // mesh.cpp:103-133
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
                    d = lp - is.p;                                                    // shape.cpp:64-78
                    const float dist2 = dot(d, d);
                    dist = __builtin_sqrtf(dist2);
                    d = d / dist;
                    const float dp = fabsf(dot(d, ln));
                    pdf *= (dp != 0.f) ? dist2 / dp : 0.f;
                    if (dot(d, ln) < 0.f && pdf != 0.f) emitter_val = emitter_radiance(tb, (int) e, wl) / pdf;   // area.cpp:39-44
                    else { pdf = 0.f; emitter_val = splat(0.f); }
                }
                if (n_em > 1) { pdf *= light_sel_pdf; emitter_val = emitter_val * (float) n_em; }
                bool shadow = false;
                spec contrib = splat(0.f);
                if (pdf != 0.f) {
                    f3 wo = is.sh.to_local(d);
                    if (flipped) wo.z = -wo.z;
                    spec bsdf_val; float bsdf_pdf;
                    const BsdfRec bs = load_bsdf(tb, bsdf_id);
                    bsdf_eval_pdf<false>(tb, bs, wi_s, wo, wl, refl, &bsdf_val, &bsdf_pdf);
                    const float w = point ? 1.f : direct_weight(fN, pdf, fM, bsdf_pdf);   // a delta light: weight 1
                    contrib = emitter_val * bsdf_val * w;
                    shadow = any_nonzero(contrib);                                    // scene.cpp:91-95: an occluded sample adds nothing
                }
                if (shadow) {
                    n_shadow += 1u;
                    float t, uu, vv; uint32_t pp_;
                    const bool occluded = traverse_scene<MODE, true>(sc, g, is.p, d, tmin, dist * (1.f - MSK_SHADOW_EPS_F), stack, &t, &uu, &vv, &pp_);
                    if (!occluded) res = res + contrib / fN;
                }
            }
            // ---- BSDF samples (path.cpp:71-108)
            for (uint32_t jb = 0; jb < M; ++jb) {
                const uint32_t pb = 3u + N + 2u * jb;
                const float sample1 = counter_pair(key, pb).x;
                const f2 u2 = counter_pair(key, pb + 1u);
                f3 wo_l; bool ok; float bs_pdf, bs_eta;
                const BsdfRec bs = load_bsdf(tb, bsdf_id);
                const spec bsdf_val = bsdf_sample<false>(tb, bs, wi_s, sample1, u2, wl, refl, &wo_l, &bs_pdf, &bs_eta, &ok);
                // a failed sample traces nothing; neither does one whose value is zero at every wavelength: it can only add zeros
                const bool go = ok && any_nonzero(bsdf_val);
                if (go) {
                    n_segments += 1u;
                    if (flipped) wo_l.z = -wo_l.z;
                    const f3 wo = is.sh.to_world(wo_l);
                    const float4 hit_b = closest(is.p, wo, tmin, MSK_INF_F);
                    spec value = splat(0.f);
                    bool hit_emitter = false;
                    float emitter_pdf = 0.f;
                    if (hit_b.x != MSK_INF_F) {
                        const Interaction sb = make_interaction(tb, hit_b, wo);
                        if (sb.emitter_id >= 0) {                                     // path.cpp:82-88; records.cpp:7-14; scene.cpp:105-112
                            if (sb.wi.z > 0.f) value = emitter_radiance(tb, sb.emitter_id, wl);
                            float pdf = tb.emitters[2 * sb.emitter_id].w;
                            const float dp = fabsf(dot(wo, sb.sh.n));
                            pdf *= (dp != 0.f) ? (sb.t * sb.t) / dp : 0.f;            // shape.cpp:80-86
                            if (n_em != 1) pdf = pdf * (1.f / n_em);
                            emitter_pdf = pdf;
                            hit_emitter = true;
                        }
                    } else if (env_image) {                                           // value and density of the ray's own direction
                        const EnvView ev = env_view(tb, sc.env_emitter);
                        float sin_t;
                        const f2 uv = env_dir_to_uv(ev, wo, &sin_t);
                        value = env_radiance(ev, tb, sc.env_emitter, uv, wl);
                        emitter_pdf = env_pdf(ev, uv, sin_t);
                        if (n_em != 1) emitter_pdf = emitter_pdf * (1.f / n_em);
                        hit_emitter = true;
                    } else if (sc.env_emitter >= 0) {                                 // the `constant` sky: its own density, always
                        value = emitter_radiance(tb, sc.env_emitter, wl);
                        emitter_pdf = MSK_INV_FOUR_PI_F;
                        if (n_em != 1) emitter_pdf = emitter_pdf * (1.f / n_em);
                        hit_emitter = true;
                    }
                    if (delta) emitter_pdf = 0.f;                                     // path.cpp:104-106: BSDFFlags::Delta
                    if (hit_emitter) res = res + (bsdf_val * value * direct_weight(fM, bs_pdf, fN, emitter_pdf)) / fM;
                }
            }
            inv = emit_record<false>(sc, tb, pp, wl, res, pix, si);
        }
        n_invalid += direct_from_lanes(inv, m_have);
        have = false;
    }
#pragma unroll
    for (int o = MSK_WAVE / 2; o > 0; o >>= 1) { n_segments += (uint32_t) __shfl_xor((int) n_segments, o); n_shadow += (uint32_t) __shfl_xor((int) n_shadow, o); }
    if (lane == 0) {
        unsigned long long *c = da.counters + (size_t) (gwave % MSK_DIRECT_COUNTER_LINES) * 8u;
        atomicAdd(&c[0], end - (unsigned long long) gwave * da.per_wave); atomicAdd(&c[1], (unsigned long long) n_segments);
        atomicAdd(&c[2], (unsigned long long) n_shadow);
        if (n_invalid) atomicAdd(&c[3], (unsigned long long) n_invalid);
    }
}

}  // namespace msk
