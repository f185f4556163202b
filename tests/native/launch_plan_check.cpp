// launch_plan_check.cpp — prints what csrc/msk_plan.h decides, for tests/test_launch_plan.py to compare with a transcription
// of the ladders the plan replaced.  Knobs come from the environment, through read_render_knobs(), as in a render.
//   launch_plan_check plans                     one line per case of the cross product below: the inputs, "|", every field of the plan
//   launch_plan_check shares                    "total n_regions share[0] ... share[n_regions - 1]" per (total, n_regions)
//   launch_plan_check parts                     "n_regions n_parts skew cut[0] ... cut[n_parts]" per case
#include "../../misaki-render_amd/csrc/msk_plan.h"

#include <cstdio>
#include <cstring>

using namespace mskplan;

static void print_plan(const SceneFacts &s, const CallFacts &c, const LaunchPlan &p) {
    static const char *shade_name[4] = {"k_shade_gen_d<%d>", "k_shade_gen<%d,true>", "k_shade_gen<%d,false,true>", "k_shade_gen<%d,false>"};
    static const char *fused_name[2][4] = {{"k_wavefront_d", "k_wavefront<true>", "k_wavefront<false,true>", "k_wavefront<false>"},
                                           {"k_wavefront_h_d", "k_wavefront_h<true>", "k_wavefront_h<false,true>", "k_wavefront_h<false>"}};
    char shade[64], trace[64];
    std::snprintf(shade, sizeof shade, shade_name[p.shade_kind], (int) p.lds_tables);
    if (p.trace_family == TRACE_FAMILY_Q) std::snprintf(trace, sizeof trace, "k_trace_q");
    else std::snprintf(trace, sizeof trace, p.trace_family == TRACE_FAMILY_R ? "k_trace_r<%d>" : "k_trace<%d>", p.trace_mode);
    // the inputs, "|", the plan: the order of FIELDS in tests/test_launch_plan.py
    std::printf("%d %d %d %d %d %d %d %zu %zu %u %u %d | %d %d %d %d %s %d %zu %s %d %d %d %u %zu %zu %u %u %d %d %d %d %s %u %u %zu %u %u %d %u %u\n",
                s.trace_mode, (int) s.lds_scene, (int) s.lds_tables, (int) s.all_diffuse, (int) s.has_regular, (int) s.has_dielectric, (int) s.cull_ok,
                s.trace_lds_bytes, s.shade_lds_bytes, c.region_size, c.aov_groups, (int) c.aov_rgb,
                (int) p.lds_tables, (int) p.diffuse_only, (int) p.regular, (int) p.dielectric, shade, (int) p.sort_on, p.shade_lds_bytes,
                trace, p.trace_mode, p.refill, p.max_inner, p.queue_refill, p.trace_lds_bytes, p.bits_off, p.trace_waves, p.trace_split, (int) p.lane_refill,
                (int) p.fused_ok, (int) p.fused_h, (int) p.fused_all, fused_name[p.fused_h][p.shade_kind], p.fused_iters, p.fused_tail_pct, p.fused_lds_bytes,
                p.fused_queue_f4, p.fused_trace_f4, (int) p.cull, p.sync_group, p.timing_every);
}

static int plans() {
    const RenderKnobs knobs = read_render_knobs();
    // {shade_lds_bytes, trace_lds_bytes}: at 1024 slots per region the sort fits up to 53248 B of tables, k_trace_q's bits up to
    // 65024 B of stack + scene, and the fused kernels need the two to sum to 65536 B or less
    static const size_t lds[7][2] = {{24576, 8192}, {53248, 8192}, {53264, 8192}, {24576, 65024}, {24576, 65040}, {24576, 40960}, {24576, 40976}};
    static const uint32_t region_sizes[4] = {256, 1024, 2048, 8192};
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
                        print_plan(s, c, make_launch_plan(s, c, knobs));
                    }
    return 0;
}

static int shares() {
    for (uint32_t n : {4u, 1024u, 6144u}) {
        const unsigned long long totals[8] = {0, 1, 63, 64, 65, 64ull * n - 1, 64ull * n + 1, (1ull << 32) + 5};
        for (unsigned long long total : totals) {
            std::printf("%llu %u", total, n);
            for (uint32_t r = 0; r < n; ++r) std::printf(" %llu", region_share(total, n, r));
            std::printf("\n");
        }
    }
    return 0;
}

static int parts() {
    for (uint32_t n_regions : {1024u, 1027u, 6144u, 8192u})
        for (uint32_t n_parts = 1; n_parts <= 4; ++n_parts)
            for (uint32_t skew : {0u, 10u, 50u}) {
                std::printf("%u %u %u", n_regions, n_parts, skew);
                for (uint32_t cut : part_ranges(n_regions, n_parts, skew)) std::printf(" %u", cut);
                std::printf("\n");
            }
    return 0;
}

int main(int argc, char **argv) {
    if (argc == 2 && !std::strcmp(argv[1], "plans")) return plans();
    if (argc == 2 && !std::strcmp(argv[1], "shares")) return shares();
    if (argc == 2 && !std::strcmp(argv[1], "parts")) return parts();
    std::fprintf(stderr, "usage: launch_plan_check plans|shares|parts\n");
    return 2;
}
