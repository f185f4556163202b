// direct_plan_check.cpp — csrc/msk_plan.h: make_direct_plan, the launch geometry of the "direct" integrator (k_direct, msk_direct.h),
// over trace modes x table placements x LDS sizes x tree depths x (light_samples, bsdf_samples) x pass sizes.  Checked, for every
// case, from the plan's own contract and not from its code:
//   form        the scene's tree where k_direct has an instantiation (binary in LDS, half-float 4-wide in HBM), else the binary tree in HBM;
//   LDS         staged tables + stacks + tree fit 64 KB; the tables a block stages are the scene's placement or, where that does
//               not fit beside the tree, none; the stacks start behind the tables, on a float4;
//   stack       LDS entries + overflow entries hold what the walked tree needs; a tree in LDS never overflows;
//   geometry    records_per_wave is a multiple of 64 in [64, 1024]; records_per_launch a multiple of it; the launches cover the
//               pass exactly once; a launch traces at most max(2^26, 2048 waves x 64 lanes x rays per sample) rays (+ one wave's
//               rounding); every launch's grid has a wave for every record.
// Prints "cases N" and returns 0, or the first violation and 1.
#include "../../misaki-render_amd/csrc/msk_plan.h"

#include <cstdio>

using namespace mskplan;

int main() {
    static const size_t shade_lds[5] = {kDoneQueueBytes, kDoneQueueBytes + 4096, kDoneQueueBytes + 16384, kDoneQueueBytes + 40960, 0};
    static const size_t tree_lds[4] = {8192, 24576, 49152, 65536};
    static const uint32_t counts[8][2] = {{1, 1}, {4, 0}, {0, 4}, {3, 2}, {8, 8}, {16, 1}, {4096, 4096}, {0, 4096}};
    static const uint64_t passes[9] = {1, 63, 64, 65, 24 * 20 * 8, 512ull * 512 * 64, (1ull << 26) + 1, (1ull << 32) + 5, 0};
    static const int depths[3] = {1, 14, 40};
    unsigned long n = 0;
    for (int mode = 0; mode <= 6; ++mode)
        for (int lds_tables = 0; lds_tables < 2; ++lds_tables)
            for (size_t sl : shade_lds)
                for (size_t tl : tree_lds)
                    for (int depth : depths)
                        for (const auto &c : counts)
                            for (uint64_t total : passes) {
                                SceneFacts s;
                                s.trace_mode = mode; s.lds_scene = mode == TRACE_BIN_LDS || mode == TRACE_WIDE4_LDS; s.lds_tables = lds_tables;
                                s.shade_lds_bytes = sl;
                                const uint32_t need = tree_in_hbm(mode) ? (mode == TRACE_BIN_HBM ? depth + 2 : 3 * depth + 2) : depth + 2;
                                const uint32_t total_entries = (need + 3u) & ~3u;
                                const uint32_t lds_entries = tree_in_hbm(mode) ? std::min(total_entries, 16u) : total_entries;
                                s.trace_lds_bytes = tree_in_hbm(mode) ? (size_t) lds_entries * MSK_BLOCK * 4 + MSK_BLOCK * 16 : std::max(tl, (size_t) lds_entries * MSK_BLOCK * 4);
                                if (!tree_in_hbm(mode) && s.trace_lds_bytes > kLdsLimit) continue;       // (place_tree never makes such a scene)
                                const DirectPlan p = make_direct_plan(s, lds_entries, total_entries, depth, c[0], c[1], total);
                                const char *bad = nullptr;
                                const int want_form = mode == TRACE_BIN_LDS ? TRACE_BIN_LDS : mode == TRACE_WIDE4_HALF ? TRACE_WIDE4_HALF : TRACE_BIN_HBM;
                                if (p.form != want_form) bad = "form";
                                const size_t placed = sl >= kDoneQueueBytes ? sl - kDoneQueueBytes : 0;
                                const size_t staged = (size_t) p.stack_f4 * 16;
                                if (p.lds_bytes > kLdsLimit) bad = "lds_bytes above 64 KB";
                                if (staged != 0 && staged != placed) bad = "staged tables are neither the scene's placement nor none";
                                if (staged == 0 && placed != 0 && placed + (p.lds_bytes - staged) <= kLdsLimit) bad = "tables that fit are not staged";
                                if (p.tables_mode != (staged == 0 ? 0u : lds_tables ? 2u : 1u)) bad = "tables_mode";
                                const size_t stacks = (size_t) p.stack_entries * MSK_BLOCK * 4;
                                if (p.lds_bytes < staged + stacks + (p.form == TRACE_BIN_LDS ? 0 : (size_t) MSK_BLOCK * 16)) bad = "lds_bytes below tables + stacks";
                                if (p.form == TRACE_BIN_LDS && (p.ovf_entries != 0 || p.lds_bytes != staged + s.trace_lds_bytes)) bad = "a tree in LDS: overflow or size";
                                const uint32_t walked = p.form == TRACE_BIN_HBM ? (uint32_t) depth + 2u : p.form == TRACE_WIDE4_HALF ? total_entries : (uint32_t) depth + 2u;
                                if (p.stack_entries + p.ovf_entries < walked) bad = "stack too short for the walked tree";
                                if (p.stack_entries < 4 || p.stack_entries % 4) bad = "stack_entries";
                                if (p.rays_per_sample != 1 + c[0] + c[1]) bad = "rays_per_sample";
                                if (p.records_per_wave % MSK_WAVE || p.records_per_wave < MSK_WAVE || p.records_per_wave > kDirectMaxRecordsPerWave) bad = "records_per_wave";
                                if (p.records_per_launch == 0 || p.records_per_launch % p.records_per_wave) bad = "records_per_launch";
                                if (p.n_launches != (total + p.records_per_launch - 1) / p.records_per_launch) bad = "n_launches";
                                const uint64_t ray_bound = std::max<uint64_t>(kDirectRaysPerLaunch, kDirectMinWaves * MSK_WAVE * p.rays_per_sample);
                                const uint64_t in_launch = std::min<uint64_t>(p.records_per_launch, total);
                                if (in_launch * p.rays_per_sample > ray_bound + (uint64_t) p.records_per_wave * p.rays_per_sample) bad = "rays per launch";
                                if ((uint64_t) p.grid_blocks(in_launch) * kWavesPerBlock * p.records_per_wave < in_launch) bad = "grid does not cover the launch";
                                if (in_launch && (uint64_t) (p.grid_blocks(in_launch) - 1) * kWavesPerBlock * p.records_per_wave >= in_launch) bad = "grid has an idle block";
                                if (bad) {
                                    std::printf("violation: %s: mode %d lds_tables %d shade_lds %zu tree_lds %zu depth %d N %u M %u records %llu\n", bad, mode, lds_tables, sl, tl,
                                                depth, c[0], c[1], (unsigned long long) total);
                                    return 1;
                                }
                                ++n;
                            }
    std::printf("cases %lu\n", n);
    return 0;
}
