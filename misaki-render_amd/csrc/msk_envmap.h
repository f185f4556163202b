// msk_envmap.h — host side of the `envmap` emitter (MSK_EMITTER_ENVMAP, include/msk_gpu.h: msk_envmap_desc): validation of the
// descriptor and construction of the cumulative tables the device samples light directions from.  Plain C++, no HIP: a native
// check compiles it on its own (tests/native/envmap_cdf_check.cpp).
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

namespace mskenv {

struct Tables {
    std::vector<float> cond;      // height rows of width + 1 entries: row j's cumulative distribution over its columns, 0 .. 1
    std::vector<float> marg;      // height + 1 entries: the cumulative distribution over the rows, 0 .. 1
};

// nullptr, or what is wrong with the weights (one per texel, row-major)
inline const char *check_weights(const float *w, uint32_t width, uint32_t height) {
    bool mass = false;
    for (size_t k = 0; k < (size_t) width * height; ++k) {
        if (!std::isfinite(w[k]) || w[k] < 0.f) return "envmap: weights must be finite and non-negative";
        mass |= w[k] > 0.f;
    }
    return mass ? nullptr : "envmap: the weights are all zero (no probability mass found)";
}

// A cumulative table of n + 1 floats from n non-negative weights: sums in double, entry k = float(sum of the first k / total),
// the last entry exactly 1.  Rounding is monotone, so the table is; a cell of zero weight repeats its predecessor's entry, and a
// positive cell whose share is below the table's resolution does too: neither is ever drawn (the search returns a cell with
// cdf[k] <= u < cdf[k + 1]) and both have pmf 0.  total == 0 (a row of no weight): 0 .. 0 1, never reached through the marginal.
inline void cumulative(const double *w, uint32_t n, float *out) {
    double total = 0.0;
    for (uint32_t k = 0; k < n; ++k) total += w[k];
    double run = 0.0;
    out[0] = 0.f;
    for (uint32_t k = 0; k < n; ++k) {
        run += w[k];
        out[k + 1] = total > 0.0 ? (float) (run / total) : 0.f;
    }
    out[n] = 1.f;      // (run == total there, bit for bit: the same additions; only a table of no weight needs the store)
}

inline Tables build_tables(const float *weights, uint32_t width, uint32_t height) {
    Tables t;
    t.cond.assign((size_t) height * (width + 1), 0.f);
    t.marg.assign((size_t) height + 1, 0.f);
    std::vector<double> row(width), rows(height);
    for (uint32_t j = 0; j < height; ++j) {
        double sum = 0.0;
        for (uint32_t i = 0; i < width; ++i) { row[i] = (double) weights[(size_t) j * width + i]; sum += row[i]; }
        rows[j] = sum;
        cumulative(row.data(), width, &t.cond[(size_t) j * (width + 1)]);
    }
    cumulative(rows.data(), height, t.marg.data());
    return t;
}

// to_world (row-major 3x3) must be a rotation: orthonormal rows within 1e-4 per entry of R R^T, determinant > 0
inline bool is_rotation(const float *r) {
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) {
            const double d = (double) r[a * 3] * r[b * 3] + (double) r[a * 3 + 1] * r[b * 3 + 1] + (double) r[a * 3 + 2] * r[b * 3 + 2];
            if (!(std::fabs(d - (a == b ? 1.0 : 0.0)) <= 1e-4)) return false;
        }
    const double det = (double) r[0] * ((double) r[4] * r[8] - (double) r[5] * r[7]) - (double) r[1] * ((double) r[3] * r[8] - (double) r[5] * r[6]) +
                       (double) r[2] * ((double) r[3] * r[7] - (double) r[4] * r[6]);
    return det > 0.0;
}

}  // namespace mskenv
