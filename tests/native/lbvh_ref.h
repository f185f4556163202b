// lbvh_ref.h — a scalar CPU twin of the device-side BVH builder (misaki-render_amd/csrc/msk_lbvh.hip), the checks of a built tree
// that do not rest on the twin, and the inputs both check programs run (lbvh_tree_check.cpp on any box, lbvh_tree_check.hip on
// the GPU).  Plain C++17, no HIP.
//
// The twin takes what msklbvh::build takes (host pointers) and returns what it writes.  It goes by another route wherever there
// is one: by-value min / max instead of fminf / fmaxf, a bit loop instead of the multiply-and-mask interleave, std::sort instead
// of the radix sort, a top-down recursion on the highest differing key bit instead of Karras's binary searches, a recursive
// union instead of the arrival counters, a running count instead of the scan.  The builder's arithmetic is fp32 min / max, one
// rounded subtraction or addition of the padding and integers, so the two are compared bit for bit.
//
// Signed zeros: fminf(+0, -0) and a by-value min may return zeros of different sign.  What is compared are the PADDED floats,
// and with a pad > 0 the sign of a zero does not survive the subtraction; every input keeps box_pad > 0 and tri_pad > 0.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <functional>
#include <random>
#include <string>
#include <vector>
#include "../../misaki-render_amd/csrc/msk_bvh.h"
#include "../../misaki-render_amd/csrc/msk_layout.h"

namespace lbvhref {

static constexpr uint32_t kLeafBit = 0x80000000u;

struct Input {                   // msklbvh::Input with host pointers
    const float *tri_verts;      // 12 floats per triangle: p0 | mesh (uint bits), p1 | -, p2 | -
    uint32_t n_tris;
    float lo[3], hi[3];          // the Morton grid
    float box_pad, tri_pad;
    uint32_t leaf_size;
    const int32_t *mesh_info;    // 4 ints per mesh, [0] = BSDF index
    const float *bsdfs;          // bsdf_f4 * 4 floats per BSDF, word 0 = type (int bits)
    uint32_t n_bsdfs, bsdf_f4, class_shift;
};

struct Tree {
    std::vector<float> nodes, tris, bounds;        // 16 / 16 / 8 floats per record
    uint32_t root_ref = 0, n_nodes = 0;
    int depth = 0;
    // the uncollapsed hierarchy (inner node i of n - 1), for the comparison with k_hierarchy's loops
    std::vector<uint64_t> keys;                    // sorted
    std::vector<uint32_t> first, last, left, right, height;
};

static inline float vmin2(float a, float b) { return b < a ? b : a; }
static inline float vmax2(float a, float b) { return a < b ? b : a; }
static inline uint32_t f2u(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
static inline float u2f(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }

struct Box3 { float lo[3], hi[3]; };
static inline Box3 tri_box_by_value(const float *v) {                 // v: 12 floats
    Box3 b;
    for (int a = 0; a < 3; ++a) {
        b.lo[a] = vmin2(v[a], vmin2(v[4 + a], v[8 + a]));
        b.hi[a] = vmax2(v[a], vmax2(v[4 + a], v[8 + a]));
    }
    return b;
}
static inline Box3 box_union(const Box3 &x, const Box3 &y) {
    Box3 u;
    for (int a = 0; a < 3; ++a) { u.lo[a] = vmin2(x.lo[a], y.lo[a]); u.hi[a] = vmax2(x.hi[a], y.hi[a]); }
    return u;
}

// the cell of a box centre along one axis: the fp32 operations of k_prims in their order
static inline uint32_t morton_cell(float lo, float hi, float grid_lo, float inv) {
    const float c = (0.5f * (lo + hi) - grid_lo) * inv;
    const float s = c * 1024.f;
    const float q = s > 0.f ? (s < 1023.f ? s : 1023.f) : 0.f;        // fminf(fmaxf(s, 0), 1023); a NaN goes to 0 there as well
    return (uint32_t) q;
}
static inline uint32_t morton30(uint32_t qx, uint32_t qy, uint32_t qz) {
    uint32_t code = 0;
    for (int b = 0; b < 10; ++b) {
        code |= ((qx >> b) & 1u) << (3 * b + 2);
        code |= ((qy >> b) & 1u) << (3 * b + 1);
        code |= ((qz >> b) & 1u) << (3 * b);
    }
    return code;
}
static inline void grid_inverse(const Input &in, float inv[3]) {
    for (int a = 0; a < 3; ++a) { const float ex = in.hi[a] - in.lo[a]; inv[a] = ex > 0.f ? 1.f / ex : 0.f; }
}

// triangle record and bounds of prim p at leaf position k, as k_tris writes them
static inline void emit_triangle(const Input &in, uint32_t prim, float *t, float *bb) {
    const float *v = in.tri_verts + (size_t) prim * 12;
    const float p[9] = {v[0], v[1], v[2], v[4], v[5], v[6], v[8], v[9], v[10]};
    const float e1[3] = {p[0] - p[3], p[1] - p[4], p[2] - p[5]};
    const float e2[3] = {p[6] - p[0], p[7] - p[1], p[8] - p[2]};
    const float ng[3] = {e2[1] * e1[2] - e2[2] * e1[1], e2[2] * e1[0] - e2[0] * e1[2], e2[0] * e1[1] - e2[1] * e1[0]};
    uint32_t word = prim;
    if (in.class_shift) {
        const int32_t bsdf = in.mesh_info[(size_t) f2u(v[3]) * 4];
        const uint32_t cls = (bsdf >= 0 && (uint32_t) bsdf < in.n_bsdfs) ? f2u(in.bsdfs[(size_t) bsdf * in.bsdf_f4 * 4]) : 0u;
        word |= (cls & 3u) << in.class_shift;
    }
    t[0] = p[0]; t[1] = p[1]; t[2] = p[2]; t[3] = u2f(word);
    for (int a = 0; a < 3; ++a) { t[4 + a] = e1[a]; t[8 + a] = e2[a]; t[12 + a] = ng[a]; }
    t[7] = t[11] = t[15] = 0.f;
    for (int a = 0; a < 3; ++a) {
        const float w0 = p[a], w1 = p[a] - e1[a], w2 = p[a] + e2[a];
        bb[a] = std::min(w0, std::min(w1, w2)) - in.tri_pad;
        bb[4 + a] = std::max(w0, std::max(w1, w2)) + in.tri_pad;
    }
    bb[3] = bb[7] = 0.f;
}

static inline Tree build(const Input &in) {
    Tree T;
    const uint32_t n = in.n_tris;
    if (n == 0) return T;
    const uint32_t leaf_size = in.leaf_size < 1 ? 1 : in.leaf_size;
    float inv[3]; grid_inverse(in, inv);
    std::vector<Box3> tb(n);
    T.keys.resize(n);
    for (uint32_t i = 0; i < n; ++i) {
        tb[i] = tri_box_by_value(in.tri_verts + (size_t) i * 12);
        uint32_t q[3];
        for (int a = 0; a < 3; ++a) q[a] = morton_cell(tb[i].lo[a], tb[i].hi[a], in.lo[a], inv[a]);
        T.keys[i] = ((uint64_t) morton30(q[0], q[1], q[2]) << 32) | i;
    }
    std::sort(T.keys.begin(), T.keys.end());
    T.tris.resize((size_t) n * 16); T.bounds.resize((size_t) n * 8);
    for (uint32_t k = 0; k < n; ++k) emit_triangle(in, (uint32_t) T.keys[k], &T.tris[(size_t) k * 16], &T.bounds[(size_t) k * 8]);
    if (n == 1 || n <= leaf_size) { T.root_ref = kLeafBit | n; return T; }

    const uint32_t ni = n - 1;
    T.first.assign(ni, 0); T.last.assign(ni, 0); T.left.assign(ni, 0); T.right.assign(ni, 0); T.height.assign(ni, 0);
    std::vector<Box3> nb(ni);
    std::vector<uint8_t> made(ni, 0);
    // node `me` over the keys [lo, hi], lo < hi: returns its box, leaves its height behind
    std::function<Box3(uint32_t, uint32_t, uint32_t)> rec = [&](uint32_t me, uint32_t lo, uint32_t hi) -> Box3 {
        const uint64_t diff = T.keys[lo] ^ T.keys[hi];                       // never 0: the index half makes every key distinct
        int bit = 63; while (!((diff >> bit) & 1ull)) --bit;
        uint32_t gamma = lo;                                                 // the last key with that bit clear
        while (!((T.keys[gamma + 1] >> bit) & 1ull)) ++gamma;
        made[me] = 1;
        T.first[me] = lo; T.last[me] = hi;
        uint32_t hl = 0, hr = 0;
        Box3 a, b;
        if (lo == gamma) { T.left[me] = gamma | kLeafBit; a = tb[(uint32_t) T.keys[gamma]]; }
        else { T.left[me] = gamma; a = rec(gamma, lo, gamma); hl = T.height[gamma]; }
        if (hi == gamma + 1) { T.right[me] = (gamma + 1) | kLeafBit; b = tb[(uint32_t) T.keys[gamma + 1]]; }
        else { T.right[me] = gamma + 1; b = rec(gamma + 1, gamma + 1, hi); hr = T.height[gamma + 1]; }
        T.height[me] = 1u + std::max(hl, hr);
        return nb[me] = box_union(a, b);
    };
    rec(0, 0, n - 1);

    // keep, renumber, emit
    std::vector<uint32_t> new_index(ni, 0);
    uint32_t kept = 0;
    for (uint32_t i = 0; i < ni; ++i) { new_index[i] = kept; if (T.last[i] - T.first[i] + 1u > leaf_size) ++kept; }
    T.n_nodes = kept;
    T.nodes.assign((size_t) kept * 16, 0.f);
    auto final_ref = [&](uint32_t ref) -> uint32_t {
        if (ref & kLeafBit) return kLeafBit | ((ref & ~kLeafBit) << 5) | 1u;
        const uint32_t cnt = T.last[ref] - T.first[ref] + 1u;
        return cnt <= leaf_size ? (kLeafBit | (T.first[ref] << 5) | cnt) : new_index[ref];
    };
    auto child = [&](uint32_t ref) { return (ref & kLeafBit) ? tb[(uint32_t) T.keys[ref & ~kLeafBit]] : nb[ref]; };
    for (uint32_t i = 0; i < ni; ++i) {
        if (!(T.last[i] - T.first[i] + 1u > leaf_size)) continue;
        Box3 a = child(T.left[i]), b = child(T.right[i]);
        for (int x = 0; x < 3; ++x) { a.lo[x] -= in.box_pad; a.hi[x] += in.box_pad; b.lo[x] -= in.box_pad; b.hi[x] += in.box_pad; }
        float *o = &T.nodes[(size_t) new_index[i] * 16];
        o[0] = a.lo[0]; o[1] = b.lo[0]; o[2] = a.lo[1]; o[3] = b.lo[1]; o[4] = a.lo[2]; o[5] = b.lo[2];
        o[6] = a.hi[0]; o[7] = b.hi[0]; o[8] = a.hi[1]; o[9] = b.hi[1]; o[10] = a.hi[2]; o[11] = b.hi[2];
        o[12] = u2f(final_ref(T.left[i])); o[13] = u2f(final_ref(T.right[i])); o[14] = 0.f; o[15] = 0.f;
    }
    T.root_ref = 0;
    T.depth = (int) T.height[0];
    return T;
}

// ------------------------------------------------------------------------------------------
// Checks of any (nodes, tris, bounds, root_ref, n_nodes, depth) against the input triangles alone
// ------------------------------------------------------------------------------------------
struct TreeView { const float *nodes, *tris, *bounds; uint32_t root_ref, n_nodes; int depth; };
struct Walked { int depth = 0; uint32_t leaves = 0; };

// the host builder's records of the same triangles, by prim (the two builders order leaves differently)
struct HostRecords {
    std::vector<float> tris, bounds;               // indexed by prim
    explicit HostRecords(const Input &in) {
        const uint32_t n = in.n_tris;
        std::vector<float> pos((size_t) n * 9);
        for (uint32_t t = 0; t < n; ++t)
            for (int v = 0; v < 3; ++v)
                for (int a = 0; a < 3; ++a) pos[(size_t) t * 9 + v * 3 + a] = in.tri_verts[(size_t) t * 12 + v * 4 + a];
        const mskbvh::Built b = mskbvh::build(pos.data(), n, in.tri_pad);
        tris.resize((size_t) n * 16); bounds.resize((size_t) n * 8);
        for (uint32_t k = 0; k < n; ++k) {
            const uint32_t prim = f2u(b.tris[(size_t) k * 16 + 3]);
            std::memcpy(&tris[(size_t) prim * 16], &b.tris[(size_t) k * 16], 64);
            std::memcpy(&bounds[(size_t) prim * 8], &b.bounds[(size_t) k * 8], 32);
        }
    }
};

// "" or the first violation.  *walked: the emitted tree's depth (inner nodes on the longest root-to-leaf path) and leaf count.
static inline std::string check_tree(const Input &in, const TreeView &t, const HostRecords &host, Walked *walked) {
    char msg[256];
    const uint32_t n = in.n_tris, leaf_size = in.leaf_size < 1 ? 1 : in.leaf_size;
    *walked = Walked();
    if (n == 0) return (t.root_ref == 0 && t.n_nodes == 0 && t.depth == 0) ? "" : "n = 0: a result that is not empty";
    const uint32_t class_mask = in.class_shift ? ~(3u << in.class_shift) : ~0u;
    // triangles, class bits, permutation
    std::vector<uint8_t> seen(n, 0);
    for (uint32_t k = 0; k < n; ++k) {
        const uint32_t word = f2u(t.tris[(size_t) k * 16 + 3]), prim = word & class_mask;
        if (prim >= n || seen[prim]) { snprintf(msg, sizeof msg, "triangle record %u: prim %u out of range or held twice", k, prim); return msg; }
        seen[prim] = 1;
        uint32_t want = 0;
        if (in.class_shift) {
            const int32_t bsdf = in.mesh_info[(size_t) f2u(in.tri_verts[(size_t) prim * 12 + 3]) * 4];
            if (bsdf >= 0 && (uint32_t) bsdf < in.n_bsdfs) want = (f2u(in.bsdfs[(size_t) bsdf * in.bsdf_f4 * 4]) & 3u) << in.class_shift;
        }
        if ((word & ~class_mask) != want) { snprintf(msg, sizeof msg, "triangle record %u (prim %u): class bits %#x, expected %#x", k, prim, word & ~class_mask, want); return msg; }
        float rec[16]; std::memcpy(rec, &host.tris[(size_t) prim * 16], 64);
        rec[3] = u2f(word);                                            // (the host builder writes the bare prim; its classes come later)
        if (f2u(host.tris[(size_t) prim * 16 + 3]) != prim) return "host record with a foreign prim word";
        if (std::memcmp(rec, &t.tris[(size_t) k * 16], 64)) { snprintf(msg, sizeof msg, "triangle record %u (prim %u) differs from the host builder's", k, prim); return msg; }
        if (std::memcmp(&host.bounds[(size_t) prim * 8], &t.bounds[(size_t) k * 8], 32)) { snprintf(msg, sizeof msg, "bounds %u (prim %u) differ from the host builder's", k, prim); return msg; }
    }
    // partition and boxes: one walk from the root
    std::vector<uint8_t> visited(t.n_nodes, 0), covered(n, 0);
    std::string err;
    int max_depth = 0; uint32_t leaves = 0;
    // returns the by-value union of the subtree's triangle boxes; depth = inner nodes above
    std::function<Box3(uint32_t, int)> walk = [&](uint32_t ref, int depth) -> Box3 {
        Box3 u{{INFINITY, INFINITY, INFINITY}, {-INFINITY, -INFINITY, -INFINITY}};
        if (!err.empty()) return u;
        if (ref & kLeafBit) {
            const uint32_t first = (ref & ~kLeafBit) >> 5, count = ref & 31u;
            max_depth = std::max(max_depth, depth); ++leaves;
            if (count < 1 || count > leaf_size || (uint64_t) first + count > n) { snprintf(msg, sizeof msg, "leaf %#x: count %u (leaf size %u) or range past %u", ref, count, leaf_size, n); err = msg; return u; }
            for (uint32_t k = first; k < first + count; ++k) {
                if (covered[k]) { snprintf(msg, sizeof msg, "triangle record %u lies in two leaves", k); err = msg; return u; }
                covered[k] = 1;
                u = box_union(u, tri_box_by_value(in.tri_verts + (size_t) (f2u(t.tris[(size_t) k * 16 + 3]) & class_mask) * 12));
            }
            return u;
        }
        if (ref >= t.n_nodes) { snprintf(msg, sizeof msg, "node reference %u with %u nodes", ref, t.n_nodes); err = msg; return u; }
        if (visited[ref]) { snprintf(msg, sizeof msg, "node %u reached twice", ref); err = msg; return u; }
        visited[ref] = 1;
        const float *o = t.nodes + (size_t) ref * 16;
        for (int c = 0; c < 2; ++c) {
            const Box3 b = walk(f2u(o[12 + c]), depth + 1);
            if (!err.empty()) return u;
            for (int a = 0; a < 3; ++a) {
                const float lo = b.lo[a] - in.box_pad, hi = b.hi[a] + in.box_pad;
                if (f2u(lo) != f2u(o[2 * a + c]) || f2u(hi) != f2u(o[6 + 2 * a + c])) {
                    snprintf(msg, sizeof msg, "node %u child %d axis %d: box [%.9g, %.9g], the padded union of its triangles is [%.9g, %.9g]", ref, c, a, o[2 * a + c], o[6 + 2 * a + c], lo, hi);
                    err = msg; return u;
                }
            }
            u = box_union(u, b);
        }
        if (f2u(o[14]) != 0 || f2u(o[15]) != 0) { snprintf(msg, sizeof msg, "node %u: words 14 / 15 are not zero", ref); err = msg; }
        return u;
    };
    walk(t.root_ref, 0);
    if (!err.empty()) return err;
    for (uint32_t i = 0; i < t.n_nodes; ++i) if (!visited[i]) { snprintf(msg, sizeof msg, "node %u of %u is never reached", i, t.n_nodes); return msg; }
    for (uint32_t k = 0; k < n; ++k) if (!covered[k]) { snprintf(msg, sizeof msg, "triangle record %u lies in no leaf", k); return msg; }
    walked->depth = max_depth; walked->leaves = leaves;
    if (t.depth < max_depth) { snprintf(msg, sizeof msg, "depth %d, the emitted tree is %d deep", t.depth, max_depth); return msg; }
    return "";
}

// ------------------------------------------------------------------------------------------
// Inputs
// ------------------------------------------------------------------------------------------
struct Case {
    std::string name;
    std::vector<float> verts;                      // 12 floats per triangle
    std::vector<int32_t> mesh_info;                // 6 meshes: BSDF 0, 1, 2, 3, 7 (out of range), -1
    std::vector<float> bsdfs;
    Input in;
    bool staircase = false;
    void finish(uint32_t leaf, uint32_t class_shift, const float *lo, const float *hi) {
        const uint32_t n = (uint32_t) (verts.size() / 12);
        static const int32_t which[6] = {0, 1, 2, 3, 7, -1};
        mesh_info.assign(6 * 4, 0);
        for (int m = 0; m < 6; ++m) mesh_info[m * 4] = which[m];
        const uint32_t bsdf_f4 = MSK_BSDF_F4;
        static const uint32_t types[4] = {1, 2, 3, 4};                     // (type 4 has class 0: two bits)
        bsdfs.assign((size_t) 4 * bsdf_f4 * 4, 0.25f);
        for (int b = 0; b < 4; ++b) bsdfs[(size_t) b * bsdf_f4 * 4] = u2f(types[b]);
        float glo[3] = {INFINITY, INFINITY, INFINITY}, ghi[3] = {-INFINITY, -INFINITY, -INFINITY};
        for (uint32_t t = 0; t < n; ++t) {
            verts[(size_t) t * 12 + 3] = u2f(t % 6u);
            for (int v = 0; v < 3; ++v)
                for (int a = 0; a < 3; ++a) { const float q = verts[(size_t) t * 12 + v * 4 + a]; glo[a] = std::min(glo[a], q); ghi[a] = std::max(ghi[a], q); }
        }
        if (n == 0) for (int a = 0; a < 3; ++a) { glo[a] = 0.f; ghi[a] = 1.f; }
        // the padding as the library derives it (msk_scene_tables.h: pack_bounds): 0.5e-5 of max(diagonal, largest |coordinate|)
        const float ex = ghi[0] - glo[0], ey = ghi[1] - glo[1], ez = ghi[2] - glo[2];
        const float diag = std::sqrt(ex * ex + (ey * ey + ez * ez));
        float amax = 0.f;
        for (int a = 0; a < 3; ++a) amax = std::max(amax, std::max(std::fabs(glo[a]), std::fabs(ghi[a])));
        in.tri_verts = verts.data(); in.n_tris = n;
        for (int a = 0; a < 3; ++a) { in.lo[a] = lo ? lo[a] : glo[a]; in.hi[a] = hi ? hi[a] : ghi[a]; }
        in.tri_pad = (0.5f * 1e-5f) * std::max(diag, amax); in.box_pad = 2.f * in.tri_pad;
        in.leaf_size = leaf;
        in.mesh_info = mesh_info.data(); in.bsdfs = bsdfs.data(); in.n_bsdfs = 4; in.bsdf_f4 = bsdf_f4; in.class_shift = class_shift;
    }
    Case() = default;
    Case(const Case &) = delete;                   // `in` points into this object's vectors
};

static inline void push_tri(std::vector<float> &v, const float p[9]) {
    for (int k = 0; k < 3; ++k) { v.push_back(p[k * 3]); v.push_back(p[k * 3 + 1]); v.push_back(p[k * 3 + 2]); v.push_back(0.f); }
}

// family a: the soup of bvh_quant_check.cpp — sizes over two decades, slivers, axis-aligned triangles
static inline void soup(std::vector<float> &v, uint32_t n, uint32_t seed, float world) {
    std::mt19937 rng(seed);
    std::uniform_real_distribution<float> u(-1.f, 1.f);
    for (uint32_t t = 0; t < n; ++t) {
        float c[3] = {u(rng) * 300.f, u(rng) * 300.f, u(rng) * 300.f};
        const float size = std::pow(10.f, u(rng) * 1.2f);
        const int kind = (int) (rng() % 10);
        float p[9];
        for (int k = 0; k < 3; ++k)
            for (int a = 0; a < 3; ++a) {
                float d = u(rng) * size;
                if (kind == 0 && a == (int) (t % 3)) d = 0.f;
                if (kind == 1 && k == 2) d *= 1e-4f;
                p[k * 3 + a] = (c[a] + d) * world;
            }
        push_tri(v, p);
    }
}
// family b: every triangle's box has the same centre (0, 0, 0): all Morton codes equal
static inline void same_centre(std::vector<float> &v, uint32_t n, uint32_t seed) {
    std::mt19937 rng(seed);
    std::uniform_real_distribution<float> u(0.01f, 1.f);
    for (uint32_t t = 0; t < n; ++t) {
        const float s = u(rng);
        const float p[9] = {-s, -s, -s, s, -s, s, -s, s, s};
        push_tri(v, p);
    }
}
// family c: five cells, each holding exact duplicates of one triangle
static inline void duplicates(std::vector<float> &v, uint32_t n) {
    static const float proto[5][9] = {{-0.9f, -0.9f, -0.9f, -0.8f, -0.9f, -0.9f, -0.9f, -0.8f, -0.85f}, {0.5f, 0.5f, 0.5f, 0.6f, 0.5f, 0.55f, 0.5f, 0.6f, 0.5f},
                                      {0.f, -0.f, 0.f, 0.1f, 0.f, -0.f, -0.f, 0.1f, 0.05f}, {0.9f, -0.9f, 0.2f, 0.8f, -0.9f, 0.2f, 0.9f, -0.8f, 0.25f},
                                      {-0.3f, 0.7f, -0.6f, -0.2f, 0.7f, -0.6f, -0.3f, 0.8f, -0.6f}};
    for (uint32_t t = 0; t < n; ++t) push_tri(v, proto[t % 5]);
}
// family d: the staircase — cluster r sits in the middle of cell (1023 >> ((r+2)/3), 1023 >> ((r+1)/3), 1023 >> (r/3)) of the box
// [origin, origin + S]^3, every triangle a tenth of a cell wide, triangle i in cluster i % 31: a chain of 30 splits
static inline void staircase(std::vector<float> &v, uint32_t n, uint32_t seed, float origin, float S) {
    std::mt19937 rng(seed);
    std::uniform_real_distribution<float> u(-1.f, 1.f);
    const float cell = S / 1024.f;
    for (uint32_t t = 0; t < n; ++t) {
        const uint32_t r = t % 31u;
        const uint32_t q[3] = {1023u >> ((r + 2) / 3), 1023u >> ((r + 1) / 3), 1023u >> (r / 3)};
        float p[9];
        for (int k = 0; k < 3; ++k)
            for (int a = 0; a < 3; ++a) p[k * 3 + a] = origin + ((float) q[a] + 0.5f) * cell + u(rng) * 0.05f * cell;
        push_tri(v, p);
    }
}
// family e: planar — every z is a zero (of either sign): extent 0 on that axis
static inline void planar(std::vector<float> &v, uint32_t n, uint32_t seed) {
    std::mt19937 rng(seed);
    std::uniform_real_distribution<float> u(-1.f, 1.f);
    for (uint32_t t = 0; t < n; ++t) {
        const float cx = u(rng) * 10.f, cy = u(rng) * 10.f;
        float p[9];
        for (int k = 0; k < 3; ++k) { p[k * 3] = cx + u(rng) * 0.3f; p[k * 3 + 1] = cy + u(rng) * 0.3f; p[k * 3 + 2] = (rng() & 1u) ? 0.f : -0.f; }
        push_tri(v, p);
    }
}
// ... and an extent of one ulp: every z is 3 or the float after it
static inline void one_ulp(std::vector<float> &v, uint32_t n, uint32_t seed) {
    std::mt19937 rng(seed);
    std::uniform_real_distribution<float> u(-1.f, 1.f);
    for (uint32_t t = 0; t < n; ++t) {
        const float cx = u(rng) * 10.f, cy = u(rng) * 10.f;
        float p[9];
        for (int k = 0; k < 3; ++k) { p[k * 3] = cx + u(rng) * 0.3f; p[k * 3 + 1] = cy + u(rng) * 0.3f; p[k * 3 + 2] = (rng() & 1u) ? 3.f : std::nextafterf(3.f, 4.f); }
        push_tri(v, p);
    }
}

static const char *const kFamilies[] = {"a1", "a1e-3", "a1e3", "b", "c", "d0_1", "d0_100", "dm_1", "dm_100", "e", "e_ulp", "f_small", "f_large"};
static constexpr int kNumFamilies = 13;

static inline void make_case(Case &c, int family, uint32_t n, uint32_t leaf, uint32_t class_shift) {
    char name[96];
    snprintf(name, sizeof name, "%-8s n %6u leaf %u class %2u", kFamilies[family], n, leaf, class_shift);
    c.name = name;
    const uint32_t seed = 1000u * (uint32_t) family + n;
    float lo[3], hi[3];
    const float *plo = nullptr, *phi = nullptr;
    auto cube = [&](float a, float b) { for (int k = 0; k < 3; ++k) { lo[k] = a; hi[k] = b; } plo = lo; phi = hi; };
    switch (family) {
    case 0: soup(c.verts, n, seed, 1.f); break;
    case 1: soup(c.verts, n, seed, 1e-3f); break;
    case 2: soup(c.verts, n, seed, 1e3f); break;
    case 3: same_centre(c.verts, n, seed); cube(-1.f, 1.f); break;
    case 4: duplicates(c.verts, n); cube(-1.f, 1.f); break;
    case 5: staircase(c.verts, n, seed, 0.f, 1.f); cube(0.f, 1.f); c.staircase = true; break;
    case 6: staircase(c.verts, n, seed, 0.f, 100.f); cube(0.f, 100.f); c.staircase = true; break;
    case 7: staircase(c.verts, n, seed, -37.5f, 1.f); cube(-37.5f, -37.5f + 1.f); c.staircase = true; break;
    case 8: staircase(c.verts, n, seed, -37.5f, 100.f); cube(-37.5f, -37.5f + 100.f); c.staircase = true; break;
    case 9: planar(c.verts, n, seed); cube(-10.3f, 10.3f); lo[2] = 0.f; hi[2] = 0.f; break;
    case 10: one_ulp(c.verts, n, seed); cube(-10.3f, 10.3f); lo[2] = 3.f; hi[2] = std::nextafterf(3.f, 4.f); break;
    case 11: soup(c.verts, n, seed, 1.f); cube(-100.f, 100.f); break;              // smaller than the geometry on every side: both clamps
    default: soup(c.verts, n, seed, 1.f); cube(-3e5f, 3e5f); break;                // a thousand times larger: a handful of cells
    }
    c.finish(leaf, class_shift, plo, phi);
}

struct CaseSpec { int family; uint32_t n, leaf, class_shift; };
// every (n, family) at the default leaf size; leaf sizes 1, 2, 4, 8 at the root-leaf boundary, 257 and 2049 for a, b, d; the
// library's class bits on a and d.  max_n trims the list (the collapse checks stop at 2049).
static inline std::vector<CaseSpec> all_cases(uint32_t max_n = 0xffffffffu) {
    std::vector<CaseSpec> out;
    const uint32_t sizes[] = {0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 2050, 4097, 70001};    // (leaf = 2 and leaf + 1 = 3 are among them)
    for (int f = 0; f < kNumFamilies; ++f)
        for (uint32_t n : sizes) if (n <= max_n) out.push_back({f, n, 2u, 0u});
    for (int f : {0, 3, 5})
        for (uint32_t leaf : {1u, 2u, 4u, 8u})
            for (uint32_t n : {leaf, leaf + 1u, 257u, 2049u}) if (n <= max_n) out.push_back({f, n, leaf, f == 3 ? 0u : (uint32_t) MSK_CLASS_SHIFT});
    for (int f : {0, 7})
        for (uint32_t n : sizes) if (n <= max_n) out.push_back({f, n, 2u, (uint32_t) MSK_CLASS_SHIFT});
    return out;
}

}  // namespace lbvhref
