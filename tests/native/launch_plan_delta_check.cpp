// launch_plan_delta_check.cpp — csrc/msk_plan.h for scenes that hold a `point` emitter or a smooth `conductor`, over the cross
// product of launch_plan_envmap_check.cpp with has_envmap added (trace modes x scene flags x AOV x region sizes x LDS sizes; knobs
// from the environment): with SceneFacts::has_delta the plan names SHADE_DELTA (k_shade_gen_p, k_wavefront_p / k_wavefront_h_p)
// whatever else the scene holds — a bitmap and an envmap included —, and every other field is what the same facts give with
// has_delta = false and has_dielectric = true (the delta instantiations are the envmap ones plus the delta light and the mirror:
// the fused kernels are not withheld, and a point light does not touch cull_ok).  A scene without either plans what it planned
// before: SHADE_ENVMAP with an envmap, else SHADE_BITMAP with a bitmap, else the older kinds.  Prints "cases N" and returns 0, or
// the first mismatch and 1.
#include "../../misaki-render_amd/csrc/msk_plan.h"

#include <cstdio>

using namespace mskplan;

#define FIELDS(X) X(lds_tables) X(diffuse_only) X(regular) X(dielectric) X(sort_on) X(shade_lds_bytes) X(trace_family) X(trace_mode) X(refill)      \
    X(max_inner) X(queue_refill) X(trace_lds_bytes) X(bits_off) X(trace_waves) X(trace_split) X(lane_refill) X(fused_ok) X(fused_h) X(fused_all) \
    X(fused_iters) X(fused_tail_pct) X(fused_lds_bytes) X(fused_queue_f4) X(fused_trace_f4) X(cull) X(sync_group) X(timing_every)

int main() {
    static_assert(SHADE_DIELECTRIC == 0 && SHADE_DIFFUSE == 1 && SHADE_REGULAR == 2 && SHADE_GENERAL == 3 && SHADE_BITMAP == 4 && SHADE_ENVMAP == 5 &&
                      SHADE_DELTA == 6,
                  "SHADE_DELTA is appended: the older values index name tables");
    const RenderKnobs knobs = read_render_knobs();
    static const size_t lds[7][2] = {{24576, 8192}, {53248, 8192}, {53264, 8192}, {24576, 65024}, {24576, 65040}, {24576, 40960}, {24576, 40976}};
    static const uint32_t region_sizes[4] = {256, 1024, 2048, 8192};
    if (SceneFacts().has_delta) { std::printf("has_delta must default to false\n"); return 1; }
    unsigned long n = 0;
    for (int mode = 0; mode <= 6; ++mode)
        for (int flags = 0; flags < 128; ++flags)
            for (int aov = 0; aov < 4; ++aov)
                for (uint32_t rs : region_sizes)
                    for (const auto &l : lds) {
                        SceneFacts s;
                        s.trace_mode = mode; s.lds_scene = mode == TRACE_BIN_LDS || mode == TRACE_WIDE4_LDS;
                        s.lds_tables = flags & 1; s.all_diffuse = flags & 2; s.has_regular = flags & 4; s.has_dielectric = flags & 8; s.cull_ok = flags & 16;
                        s.has_bitmap = flags & 32; s.has_envmap = flags & 64;
                        s.shade_lds_bytes = l[0]; s.trace_lds_bytes = l[1];
                        CallFacts c;
                        c.region_size = rs; c.aov_groups = (aov & 1) ? 2u : 0u; c.aov_rgb = (aov & 2) != 0;
                        SceneFacts sp = s, sd = s;
                        sp.has_delta = true;
                        sd.has_bitmap = false; sd.has_envmap = false; sd.has_dielectric = true;
                        const LaunchPlan e = make_launch_plan(sp, c, knobs), d = make_launch_plan(sd, c, knobs), p = make_launch_plan(s, c, knobs);
                        const char *bad = nullptr;
                        if (e.shade_kind != SHADE_DELTA) bad = "shade_kind (must be SHADE_DELTA)";
                        if (d.shade_kind != SHADE_DIELECTRIC) bad = "shade_kind of the comparison plan";
                        if (p.shade_kind == SHADE_DELTA) bad = "SHADE_DELTA without a delta light or a mirror";
                        if (s.has_envmap != (p.shade_kind == SHADE_ENVMAP)) bad = "a scene without either does not plan what it planned before (envmap)";
                        if ((s.has_bitmap && !s.has_envmap) != (p.shade_kind == SHADE_BITMAP)) bad = "a scene without either does not plan what it planned before (bitmap)";
#define X(f) if (!(e.f == d.f)) bad = #f;
                        FIELDS(X)
#undef X
                        if (bad) {
                            std::printf("mismatch in %s: mode %d flags %d aov %d region_size %u lds %zu %zu\n", bad, mode, flags, aov, rs, l[0], l[1]);
                            return 1;
                        }
                        ++n;
                    }
    std::printf("cases %lu\n", n);
    return 0;
}
