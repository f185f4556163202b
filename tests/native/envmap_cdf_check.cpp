// envmap_cdf_check.cpp — csrc/msk_envmap.h on its own (no HIP): the cumulative tables of the `envmap` emitter are monotone, start
// at 0 and end at exactly 1, a cell (and a row) of zero weight has zero pmf, a positive cell of a positive row is reachable
// unless its share is below the table's resolution, the pmfs add up to 1 within rounding; check_weights and is_rotation refuse
// what the ABI says they refuse.  Prints "cases N" and returns 0, or the first failure and 1.
#include "../../misaki-render_amd/csrc/msk_envmap.h"

#include <cstdio>
#include <cstdlib>
#include <limits>

static int fail(const char *what, unsigned w, unsigned h, unsigned j, unsigned i) {
    std::printf("FAILED: %s (image %u x %u, row %u, column %u)\n", what, w, h, j, i);
    return 1;
}

static int check(const std::vector<float> &wt, unsigned W, unsigned H) {
    const mskenv::Tables t = mskenv::build_tables(wt.data(), W, H);
    if (t.cond.size() != (size_t) H * (W + 1) || t.marg.size() != (size_t) H + 1) return fail("table sizes", W, H, 0, 0);
    if (t.marg[0] != 0.f || t.marg[H] != 1.f) return fail("marginal does not run from 0 to 1", W, H, 0, 0);
    double total = 0.0;
    std::vector<double> rows(H, 0.0);
    for (unsigned j = 0; j < H; ++j) { for (unsigned i = 0; i < W; ++i) rows[j] += wt[(size_t) j * W + i]; total += rows[j]; }
    double pmf_sum = 0.0;
    for (unsigned j = 0; j < H; ++j) {
        const float *row = &t.cond[(size_t) j * (W + 1)];
        if (!(t.marg[j + 1] >= t.marg[j])) return fail("marginal not monotone", W, H, j, 0);
        const double pr = (double) t.marg[j + 1] - (double) t.marg[j];
        if (rows[j] == 0.0 && pr != 0.0) return fail("a row of zero weight has mass", W, H, j, 0);
        if (rows[j] / total > 1e-6 && pr == 0.0) return fail("a row with a share above 1e-6 has no mass", W, H, j, 0);
        if (row[0] != 0.f || row[W] != 1.f) return fail("row table does not run from 0 to 1", W, H, j, 0);
        for (unsigned i = 0; i < W; ++i) {
            if (!(row[i + 1] >= row[i])) return fail("row table not monotone", W, H, j, i);
            const double pc = (double) row[i + 1] - (double) row[i];
            const float w = wt[(size_t) j * W + i];
            if (rows[j] > 0.0 && w == 0.f && pc != 0.0) return fail("a cell of zero weight has mass", W, H, j, i);
            if (rows[j] > 0.0 && w / rows[j] > 1e-6 && pc == 0.0) return fail("a cell with a share above 1e-6 has no mass", W, H, j, i);
            if (rows[j] > 0.0 && std::fabs(pc - w / rows[j]) > 1.2e-7) return fail("conditional pmf off by more than two roundings", W, H, j, i);
            pmf_sum += pr * pc;
        }
        if (std::fabs(pr - rows[j] / total) > 1.2e-7) return fail("marginal pmf off by more than two roundings", W, H, j, 0);
    }
    if (std::fabs(pmf_sum - 1.0) > 1e-5) return fail("the pmfs do not add up to 1", W, H, 0, 0);
    return 0;
}

int main() {
    unsigned long n = 0;
    uint64_t state = 0x9e3779b97f4a7c15ull;
    auto rnd = [&]() { state = state * 6364136223846793005ull + 1442695040888963407ull; return (float) ((state >> 40) / 16777216.0); };
    static const unsigned sizes[][2] = {{1, 1}, {2, 1}, {1, 2}, {3, 5}, {16, 8}, {40, 3}, {257, 129}};
    for (const auto &s : sizes) {
        const unsigned W = s[0], H = s[1];
        for (int kind = 0; kind < 5; ++kind) {
            std::vector<float> wt((size_t) W * H);
            for (auto &v : wt) v = kind == 0 ? 1.f : rnd() + (kind == 3 ? 1e-3f : 0.f);
            if (kind == 2) { wt[0] = 1e4f; for (unsigned i = 0; i < W; ++i) wt[(size_t) (H / 2) * W + i] = 0.f; wt[0] = 1e4f; }   // a hot texel, a row of zeros
            if (kind == 3) { for (size_t k = 0; k < wt.size(); k += 3) wt[k] = 0.f; wt.back() = 0.5f; }                              // scattered zeros
            if (kind == 4) { for (auto &v : wt) v = 0.f; wt[wt.size() - 1] = 3.f; }                                                  // all the mass in the last cell
            if (mskenv::check_weights(wt.data(), W, H)) { std::printf("FAILED: valid weights refused\n"); return 1; }
            if (check(wt, W, H)) return 1;
            ++n;
        }
    }
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float zeros[4] = {0, 0, 0, 0}, neg[4] = {1, -1, 1, 1}, infs[4] = {1, inf, 1, 1}, nans[4] = {1, 1, nan, 1};
    if (!mskenv::check_weights(zeros, 2, 2) || !mskenv::check_weights(neg, 2, 2) || !mskenv::check_weights(infs, 2, 2) || !mskenv::check_weights(nans, 2, 2)) {
        std::printf("FAILED: invalid weights accepted\n"); return 1;
    }
    const float id[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, mirror[9] = {1, 0, 0, 0, 1, 0, 0, 0, -1}, scaled[9] = {2, 0, 0, 0, 2, 0, 0, 0, 2}, shear[9] = {1, 0.1f, 0, 0, 1, 0, 0, 0, 1};
    const float c = 0.8f, s = 0.6f, rot[9] = {c, -s, 0, s, c, 0, 0, 0, 1}, bad[9] = {nan, 0, 0, 0, 1, 0, 0, 0, 1};
    if (!mskenv::is_rotation(id) || !mskenv::is_rotation(rot) || mskenv::is_rotation(mirror) || mskenv::is_rotation(scaled) || mskenv::is_rotation(shear) || mskenv::is_rotation(bad)) {
        std::printf("FAILED: is_rotation\n"); return 1;
    }
    std::printf("cases %lu\n", n);
    return 0;
}
