// launch_plan_bitmap_check.cpp — csrc/msk_plan.h for scenes that hold a `bitmap` texture, over the cross product of
// launch_plan_check.cpp (trace modes x scene flags x AOV x region sizes x LDS sizes; knobs from the environment): with
// SceneFacts::has_bitmap the plan names SHADE_BITMAP (k_shade_gen_b, k_wavefront_b / k_wavefront_h_b), and every other
// field is what the same facts give with has_bitmap = false and has_dielectric = true — the bitmap instantiations are the
// dielectric ones plus the texel lookup, and nothing else in the plan depends on the texture (the fused kernels
// are not withheld).  Prints "cases N" and returns 0, or the first mismatch and 1.
#include "../../misaki-render_amd/csrc/msk_plan.h"

#include <cstdio>

using namespace mskplan;

#define FIELDS(X) X(lds_tables) X(diffuse_only) X(regular) X(dielectric) X(sort_on) X(shade_lds_bytes) X(trace_family) X(trace_mode) X(refill)      \
    X(max_inner) X(queue_refill) X(trace_lds_bytes) X(bits_off) X(trace_waves) X(trace_split) X(lane_refill) X(fused_ok) X(fused_h) X(fused_all) \
    X(fused_iters) X(fused_tail_pct) X(fused_lds_bytes) X(fused_queue_f4) X(fused_trace_f4) X(cull) X(sync_group) X(timing_every)

int main() {
    static_assert(SHADE_DIELECTRIC == 0 && SHADE_DIFFUSE == 1 && SHADE_REGULAR == 2 && SHADE_GENERAL == 3 && SHADE_BITMAP == 4,
                  "SHADE_BITMAP is appended: the older values index name tables");
    const RenderKnobs knobs = read_render_knobs();
    static const size_t lds[7][2] = {{24576, 8192}, {53248, 8192}, {53264, 8192}, {24576, 65024}, {24576, 65040}, {24576, 40960}, {24576, 40976}};
    static const uint32_t region_sizes[4] = {256, 1024, 2048, 8192};
    if (SceneFacts().has_bitmap) { std::printf("has_bitmap must default to false\n"); return 1; }
    unsigned long n = 0;
    for (int mode = 0; mode <= 6; ++mode)
        for (int flags = 0; flags < 32; ++flags)
            for (int aov = 0; aov < 4; ++aov)
                for (uint32_t rs : region_sizes)
                    for (const auto &l : lds) {
                        SceneFacts s;
                        s.trace_mode = mode; s.lds_scene = mode == TRACE_BIN_LDS || mode == TRACE_WIDE4_LDS;
                        s.lds_tables = flags & 1; s.all_diffuse = flags & 2; s.has_regular = flags & 4; s.has_dielectric = flags & 8; s.cull_ok = flags & 16;
                        s.shade_lds_bytes = l[0]; s.trace_lds_bytes = l[1];
                        CallFacts c;
                        c.region_size = rs; c.aov_groups = (aov & 1) ? 2u : 0u; c.aov_rgb = (aov & 2) != 0;
                        SceneFacts sb = s, sd = s;
                        sb.has_bitmap = true;
                        sd.has_dielectric = true;
                        const LaunchPlan b = make_launch_plan(sb, c, knobs), d = make_launch_plan(sd, c, knobs);
                        const char *bad = nullptr;
                        if (b.shade_kind != SHADE_BITMAP) bad = "shade_kind (must be SHADE_BITMAP)";
                        if (d.shade_kind != SHADE_DIELECTRIC) bad = "shade_kind of the comparison plan";
#define X(f) if (!(b.f == d.f)) bad = #f;
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
