// bvh_contain.h — the containment checks of msk_bvh.h's wide forms, shared by bvh_quant_check.cpp (host-built trees of soups) and
// lbvh_tree_check.cpp (trees of the device builder's CPU twin): every decoded child box of nodes4q / nodes4h / nodes8 contains
// the padded full-precision box it stands for (the traversal only ever culls), the grids are the finest that span the node, unused
// slots are inverted boxes pointing at an empty leaf.  Each check returns "" or the first violation.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <functional>
#include <map>
#include <string>
#include <vector>
#include "../../misaki-render_amd/csrc/msk_bvh.h"

namespace bvhcontain {

struct Stats { double area_ratio = 0; size_t children = 0, empty = 0; double mean() const { return children ? area_ratio / children : 1.0; } };

// Built::nodes4q (byte grid, 64-byte nodes) against nodes4
static inline std::string check_nodes4q(const mskbvh::Built &b, Stats *st) {
    char msg[320];
    const size_t nn = b.nodes4.size() / 32;
    if (b.nodes4q.size() != nn * 16) { snprintf(msg, sizeof msg, "nodes4q has %zu dwords for %zu nodes", b.nodes4q.size(), nn); return msg; }
    for (size_t m = 0; m < nn; ++m) {
        const float *f = &b.nodes4[m * 32];
        const uint32_t *q = &b.nodes4q[m * 16];
        float origin[3], scale[3];
        memcpy(origin, q, 12); memcpy(&scale[0], &q[3], 4); memcpy(&scale[1], &q[4], 8);
        uint32_t refs[4]; memcpy(refs, &f[24], 16);
        for (int i = 0; i < 4; ++i) {
            double e[3], eq[3];
            for (int a = 0; a < 3; ++a) {
                const double ql = (q[6 + a] >> (8 * i)) & 255u, qh = (q[9 + a] >> (8 * i)) & 255u;
                if (refs[i] == mskbvh::kEmpty4) {
                    if (!(ql == 255 && qh == 0) || q[12 + i] != 0x80000000u) { snprintf(msg, sizeof msg, "node %zu slot %d: unused slot not inverted / not an empty leaf", m, i); return msg; }
                    continue;
                }
                if (!(scale[a] > 0.f) || !std::isfinite(scale[a])) { snprintf(msg, sizeof msg, "node %zu axis %d: scale %g", m, a, scale[a]); return msg; }
                const double lo = f[a * 4 + i], hi = f[12 + a * 4 + i];
                const double dlo = (double) origin[a] + ql * (double) scale[a], dhi = (double) origin[a] + qh * (double) scale[a];
                if (dlo > lo || dhi < hi) { snprintf(msg, sizeof msg, "node %zu child %d axis %d: [%.9g, %.9g] does not contain [%.9g, %.9g]", m, i, a, dlo, dhi, lo, hi); return msg; }
                if (dlo < lo - 1.0000001 * scale[a] || dhi > hi + 1.0000001 * scale[a]) { snprintf(msg, sizeof msg, "node %zu child %d axis %d: more than one grid cell of slack", m, i, a); return msg; }
                e[a] = hi - lo; eq[a] = dhi - dlo;
            }
            if (refs[i] == mskbvh::kEmpty4) { ++st->empty; continue; }
            if (q[12 + i] != refs[i]) { snprintf(msg, sizeof msg, "node %zu child %d: reference differs", m, i); return msg; }
            const double A = e[0] * e[1] + e[1] * e[2] + e[2] * e[0], Aq = eq[0] * eq[1] + eq[1] * eq[2] + eq[2] * eq[0];
            if (A > 0) { st->area_ratio += Aq / A; ++st->children; }
        }
    }
    return "";
}

// fp16 bits -> value, decoded here independently of the builder
static inline double half_value(uint32_t h) {
    const int e = (h >> 10) & 31, f = h & 1023;
    if (e == 31) return f ? NAN : INFINITY;
    return e ? std::ldexp(1024.0 + f, e - 25) : std::ldexp((double) f, -24);
}

// Built::nodes4h (half-float boxes, 80-byte nodes) against nodes4
static inline std::string check_nodes4h(const mskbvh::Built &b, Stats *st) {
    char msg[320];
    const size_t nn = b.nodes4.size() / 32;
    if (b.nodes4h.size() != nn * 20) { snprintf(msg, sizeof msg, "nodes4h has %zu dwords for %zu nodes", b.nodes4h.size(), nn); return msg; }
    for (size_t m = 0; m < nn; ++m) {
        const float *f = &b.nodes4[m * 32];
        const uint32_t *q = &b.nodes4h[m * 20];
        float origin[3], scale;
        memcpy(origin, q, 12); memcpy(&scale, &q[3], 4);
        int ex; if (!(scale > 0.f) || !std::isfinite(scale) || std::frexp(scale, &ex) != 0.5f) { snprintf(msg, sizeof msg, "node %zu: half scale %g is not a power of two", m, scale); return msg; }
        uint32_t refs[4]; memcpy(refs, &f[24], 16);
        for (int i = 0; i < 4; ++i) {
            double e[3], eq[3];
            for (int a = 0; a < 3; ++a) {
                const uint32_t wl = q[4 + 2 * a + i / 2], wh = q[10 + 2 * a + i / 2];
                const uint32_t hl = (wl >> (16 * (i & 1))) & 0xffffu, hh = (wh >> (16 * (i & 1))) & 0xffffu;
                if (refs[i] == mskbvh::kEmpty4) {
                    if (!(hl == 0x7bffu && hh == 0u) || q[16 + i] != 0x80000000u) { snprintf(msg, sizeof msg, "node %zu slot %d: unused half slot not inverted / not an empty leaf", m, i); return msg; }
                    continue;
                }
                if (hh != 0 && hh < 0x0400u) { snprintf(msg, sizeof msg, "node %zu child %d axis %d: subnormal upper plane", m, i, a); return msg; }
                const double lo = f[a * 4 + i], hi = f[12 + a * 4 + i];
                const double dlo = (double) origin[a] + half_value(hl) * (double) scale, dhi = (double) origin[a] + half_value(hh) * (double) scale;
                if (!(dlo <= lo && dhi >= hi) || !std::isfinite(dhi)) { snprintf(msg, sizeof msg, "node %zu child %d axis %d: half box [%.9g, %.9g] does not contain [%.9g, %.9g]", m, i, a, dlo, dhi, lo, hi); return msg; }
                // eleven bits: the slack is at most 2^-10 of the plane's own offset (or the smallest normal)
                if (dlo < lo - ((lo - origin[a]) / 1024.0 + 1e-30) || dhi > hi + std::max((hi - origin[a]) / 1024.0, 6.2e-5 * (double) scale)) { snprintf(msg, sizeof msg, "node %zu child %d axis %d: half box too loose", m, i, a); return msg; }
                e[a] = hi - lo; eq[a] = dhi - dlo;
            }
            if (refs[i] == mskbvh::kEmpty4) continue;
            if (q[16 + i] != ((refs[i] & 0x80000000u) ? refs[i] : refs[i] * 80u)) { snprintf(msg, sizeof msg, "node %zu child %d: half reference differs (a leaf's as is, an inner child's x 80)", m, i); return msg; }
            const double A = e[0] * e[1] + e[1] * e[2] + e[2] * e[0], Aq = eq[0] * eq[1] + eq[1] * eq[2] + eq[2] * eq[0];
            if (A > 0) { st->area_ratio += Aq / A; ++st->children; }
        }
    }
    return "";
}

// The padded box of every leaf reference of the binary tree, as its parent node stores it.
struct LeafBox { float lo[3], hi[3]; };
static inline std::map<uint32_t, LeafBox> binary_leaf_boxes(const mskbvh::Built &b) {
    std::map<uint32_t, LeafBox> out;
    for (size_t m = 0; m < b.nodes.size() / 16; ++m) {
        const float *n = &b.nodes[m * 16];
        uint32_t refs[2]; memcpy(refs, &n[12], 8);
        for (int c = 0; c < 2; ++c)
            if (refs[c] & 0x80000000u) { LeafBox x; for (int a = 0; a < 3; ++a) { x.lo[a] = n[2 * a + c]; x.hi[a] = n[6 + 2 * a + c]; } out[refs[c]] = x; }
    }
    return out;
}

// Built::nodes8 (byte grid on power-of-two scales, 128-byte nodes).  The form keeps no full-precision boxes, so a child's decoded
// box is held against the union of the binary tree's padded leaf boxes below it — which is the binary node's own box, the padding
// being one monotonic rounded operation — and must lie within one grid cell of it.
static inline std::string check_nodes8(const mskbvh::Built &b, Stats *st) {
    const size_t nn = b.nodes8.size() / 32;
    if (!nn) return "";
    const std::map<uint32_t, LeafBox> leaf = binary_leaf_boxes(b);
    std::string err;
    char msg[320];
    std::vector<uint8_t> visited(nn, 0);
    std::function<LeafBox(uint32_t)> walk = [&](uint32_t m) -> LeafBox {
        LeafBox u{{INFINITY, INFINITY, INFINITY}, {-INFINITY, -INFINITY, -INFINITY}};
        if (!err.empty()) return u;
        if (m >= nn || visited[m]) { snprintf(msg, sizeof msg, "8-wide node %u out of range or reached twice", m); err = msg; return u; }
        visited[m] = 1;
        const float *o = &b.nodes8[(size_t) m * 32];
        float origin[3], scale[3]; uint32_t meta, refs[8]; uint8_t q[6][8];
        memcpy(origin, &o[0], 12); memcpy(&meta, &o[3], 4); memcpy(scale, &o[4], 12); memcpy(q, &o[8], 48); memcpy(refs, &o[20], 32);
        int used = 0;
        for (int i = 0; i < 8; ++i) {
            if (refs[i] == mskbvh::kEmpty4) {
                ++st->empty;
                if ((meta >> (8 + i)) & 1u) { snprintf(msg, sizeof msg, "8-wide node %u slot %d: empty but in the mask", m, i); err = msg; return u; }
                for (int a = 0; a < 3; ++a) if (q[a][i] != 255 || q[3 + a][i] != 0) { snprintf(msg, sizeof msg, "8-wide node %u slot %d: unused slot not inverted", m, i); err = msg; return u; }
                continue;
            }
            ++used;
            if (!((meta >> (8 + i)) & 1u)) { snprintf(msg, sizeof msg, "8-wide node %u slot %d: used but not in the mask", m, i); err = msg; return u; }
            LeafBox c;
            if (refs[i] & 0x80000000u) {
                const auto it = leaf.find(refs[i]);
                if (it == leaf.end()) { snprintf(msg, sizeof msg, "8-wide node %u slot %d: leaf %#x is not a leaf of the binary tree", m, i, refs[i]); err = msg; return u; }
                c = it->second;
            } else {
                c = walk(refs[i]);
                if (!err.empty()) return u;
            }
            double e[3], eq[3];
            for (int a = 0; a < 3; ++a) {
                int ex; if (!(scale[a] > 0.f) || !std::isfinite(scale[a]) || std::frexp(scale[a], &ex) != 0.5f) { snprintf(msg, sizeof msg, "8-wide node %u axis %d: scale %g is not a power of two", m, a, scale[a]); err = msg; return u; }
                const double dlo = (double) origin[a] + q[a][i] * (double) scale[a], dhi = (double) origin[a] + q[3 + a][i] * (double) scale[a];
                if (dlo > c.lo[a] || dhi < c.hi[a]) { snprintf(msg, sizeof msg, "8-wide node %u child %d axis %d: [%.9g, %.9g] does not contain [%.9g, %.9g]", m, i, a, dlo, dhi, c.lo[a], c.hi[a]); err = msg; return u; }
                if (dlo < c.lo[a] - 1.0000001 * scale[a] || dhi > c.hi[a] + 1.0000001 * scale[a]) { snprintf(msg, sizeof msg, "8-wide node %u child %d axis %d: more than one grid cell of slack", m, i, a); err = msg; return u; }
                e[a] = (double) c.hi[a] - c.lo[a]; eq[a] = dhi - dlo;
                u.lo[a] = std::min(u.lo[a], c.lo[a]); u.hi[a] = std::max(u.hi[a], c.hi[a]);
            }
            const double A = e[0] * e[1] + e[1] * e[2] + e[2] * e[0], Aq = eq[0] * eq[1] + eq[1] * eq[2] + eq[2] * eq[0];
            if (A > 0) { st->area_ratio += Aq / A; ++st->children; }
        }
        if (used < 2) { snprintf(msg, sizeof msg, "8-wide node %u has %d children", m, used); err = msg; }
        return u;
    };
    walk(b.root_ref8);
    return err;
}

}  // namespace bvhcontain
