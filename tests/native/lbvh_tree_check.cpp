// CPU side of tests/test_lbvh_tree.py: the scalar twin of the device-side BVH builder (lbvh_ref.h) against the checks that do
// not rest on it, against a literal transcription of k_hierarchy's loops, and through the wide collapses of msk_bvh.h.
// usage: lbvh_tree_check twin              every input: the tree checks, the hierarchy against Karras's loops, the staircase's height
//        lbvh_tree_check collapse          inputs up to 2049 triangles through collapse4 (optimal, greedy) and collapse8, twin and host tree
//        lbvh_tree_check height <file>     the twin's height of the triangles in <file>: uint32 n, float lo[3], hi[3], n x 9 floats
// prints one line per case and "all ok", or "FAIL ..." lines and "FAILED"
#include <cstdio>
#include <cstdlib>
#include <set>
#include "lbvh_ref.h"
#include "bvh_contain.h"
using namespace lbvhref;

// ---- k_hierarchy (msk_lbvh.hip), thread i of n - 1, as the kernel writes it
static int delta(const uint64_t *keys, int n, int i, int j) {
    if (j < 0 || j >= n) return -1;
    return __builtin_clzll(keys[i] ^ keys[j]);
}
struct Karras { std::vector<uint32_t> first, last, left, right, height; };
static Karras karras(const std::vector<uint64_t> &k) {
    const int n = (int) k.size();
    const uint64_t *keys = k.data();
    Karras h;
    h.first.assign(n - 1, 0); h.last.assign(n - 1, 0); h.left.assign(n - 1, 0); h.right.assign(n - 1, 0); h.height.assign(n - 1, 0);
    for (int i = 0; i < n - 1; ++i) {
        const int d = (delta(keys, n, i, i + 1) - delta(keys, n, i, i - 1)) >= 0 ? 1 : -1;
        const int dmin = delta(keys, n, i, i - d);
        int lmax = 2;
        while (delta(keys, n, i, i + lmax * d) > dmin) lmax *= 2;
        int l = 0;
        for (int t = lmax / 2; t >= 1; t /= 2)
            if (delta(keys, n, i, i + (l + t) * d) > dmin) l += t;
        const int j = i + l * d;
        const int dnode = delta(keys, n, i, j);
        int s = 0, t = l;
        do {
            t = (t + 1) / 2;
            if (delta(keys, n, i, i + (s + t) * d) > dnode) s += t;
        } while (t > 1);
        const int gamma = i + s * d + (d < 0 ? -1 : 0);
        const int lo = i < j ? i : j, hi = i < j ? j : i;
        h.first[i] = (uint32_t) lo; h.last[i] = (uint32_t) hi;
        h.left[i] = lo == gamma ? (uint32_t) gamma | kLeafBit : (uint32_t) gamma;
        h.right[i] = hi == gamma + 1 ? (uint32_t) (gamma + 1) | kLeafBit : (uint32_t) (gamma + 1);
    }
    // heights without recursion: a child's range lies inside its parent's, so shorter ranges come first
    std::vector<uint32_t> order(n - 1);
    for (int i = 0; i < n - 1; ++i) order[i] = (uint32_t) i;
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return h.last[a] - h.first[a] < h.last[b] - h.first[b]; });
    for (uint32_t i : order) {
        const uint32_t hl = (h.left[i] & kLeafBit) ? 0u : h.height[h.left[i]], hr = (h.right[i] & kLeafBit) ? 0u : h.height[h.right[i]];
        h.height[i] = 1u + std::max(hl, hr);
    }
    return h;
}

static int run_twin() {
    int bad = 0;
    for (const CaseSpec &s : all_cases()) {
        Case c; make_case(c, s.family, s.n, s.leaf, s.class_shift);
        const Tree t = build(c.in);
        const HostRecords host(c.in);
        Walked w;
        std::string err = check_tree(c.in, TreeView{t.nodes.data(), t.tris.data(), t.bounds.data(), t.root_ref, t.n_nodes, t.depth}, host, &w);
        if (err.empty() && (c.in.box_pad <= 0.f || c.in.tri_pad <= 0.f)) err = "a padding that is not positive";
        if (err.empty() && t.nodes.size() != (size_t) t.n_nodes * 16) err = "n_nodes and the node array disagree";
        if (err.empty() && s.n > std::max(1u, s.leaf)) {
            const Karras k = karras(t.keys);
            if (k.first != t.first || k.last != t.last || k.left != t.left || k.right != t.right) err = "the recursion's hierarchy is not k_hierarchy's";
            else if ((int) k.height[0] != t.depth || k.height != t.height) err = "depth is not the height of the uncollapsed hierarchy";
        }
        if (err.empty() && c.staircase && s.n >= 65 && t.depth < 30) err = "a staircase of height below 30";
        printf("%s %s: depth %d walked %d nodes %u leaves %u%s%s\n", err.empty() ? "ok  " : "FAIL", c.name.c_str(), t.depth, w.depth, t.n_nodes, w.leaves, err.empty() ? "" : " — ", err.c_str());
        bad += !err.empty();
    }
    printf(bad ? "FAILED (%d)\n" : "all ok\n", bad);
    return bad ? 1 : 0;
}

// ---- the wide forms of one binary tree
static void leaf_refs2(const mskbvh::Built &b, std::multiset<uint32_t> *out) {
    if (b.root_ref & kLeafBit) { out->insert(b.root_ref); return; }
    for (size_t m = 0; m < b.nodes.size() / 16; ++m)
        for (int c = 0; c < 2; ++c) { const uint32_t r = f2u(b.nodes[m * 16 + 12 + c]); if (r & kLeafBit) out->insert(r); }
}
// leaf refs and depth (wide nodes on the longest path) by walking; slots: 4 (nodes4, refs at float 24) or 8 (nodes8, refs at float 20)
static std::string walk_wide(const std::vector<float> &nodes, uint32_t root, int slots, std::multiset<uint32_t> *refs, int *depth) {
    const size_t nn = nodes.size() / 32;
    std::vector<uint8_t> seen(nn, 0);
    std::string err;
    *depth = 0;
    std::function<void(uint32_t, int)> walk = [&](uint32_t m, int d) {
        if (!err.empty()) return;
        if (m >= nn || seen[m]) { err = "a wide node out of range or reached twice"; return; }
        seen[m] = 1;
        *depth = std::max(*depth, d);
        for (int i = 0; i < slots; ++i) {
            const uint32_t r = f2u(nodes[(size_t) m * 32 + (slots == 4 ? 24 : 20) + i]);
            if (r == mskbvh::kEmpty4) continue;
            if (r & kLeafBit) refs->insert(r); else walk(r, d + 1);
        }
    };
    if (root & kLeafBit) refs->insert(root); else walk(root, 1);
    if (err.empty()) for (size_t m = 0; m < nn; ++m) if (!seen[m]) { err = "a wide node that is never reached"; break; }
    return err;
}
// nodes4's own boxes: a leaf slot holds the binary tree's box of that leaf, bit for bit
static std::string check_nodes4_leaves(const mskbvh::Built &b) {
    const auto leaf = bvhcontain::binary_leaf_boxes(b);
    for (size_t m = 0; m < b.nodes4.size() / 32; ++m) {
        const float *f = &b.nodes4[m * 32];
        for (int i = 0; i < 4; ++i) {
            const uint32_t r = f2u(f[24 + i]);
            if (r == mskbvh::kEmpty4 || !(r & kLeafBit)) continue;
            const auto it = leaf.find(r);
            if (it == leaf.end()) return "a 4-wide leaf that the binary tree does not have";
            for (int a = 0; a < 3; ++a) if (f2u(f[a * 4 + i]) != f2u(it->second.lo[a]) || f2u(f[12 + a * 4 + i]) != f2u(it->second.hi[a])) return "a 4-wide leaf slot whose box is not the binary tree's";
        }
    }
    return "";
}
static std::string check_wide(mskbvh::Built &b, std::string *report) {
    char buf[256];
    std::multiset<uint32_t> want; leaf_refs2(b, &want);
    for (int optimal = 1; optimal >= 0; --optimal) {
        mskbvh::collapse4(b, optimal != 0);
        std::multiset<uint32_t> got; int depth = 0;
        std::string err = walk_wide(b.nodes4, b.root_ref4, 4, &got, &depth);
        if (err.empty() && got != want) err = "the 4-wide tree's leaves are not the binary tree's, each once";
        if (err.empty() && b.max_depth4 < depth) err = "max_depth4 below the walked depth";
        if (err.empty()) err = check_nodes4_leaves(b);
        bvhcontain::Stats q, h;
        const bool root_leaf = (b.root_ref & kLeafBit) != 0;
        if (err.empty() && !b.nodes4q.empty()) err = bvhcontain::check_nodes4q(b, &q);
        if (err.empty() && !b.nodes4h.empty()) err = bvhcontain::check_nodes4h(b, &h);
        if (!err.empty()) return std::string(optimal ? "collapse4 optimal: " : "collapse4 greedy: ") + err;
        snprintf(buf, sizeof buf, " | 4%s depth %d/%d byte %s half %s", optimal ? "opt" : "greedy", depth, b.max_depth4,
                 root_leaf ? "-" : b.nodes4q.empty() ? "REFUSED" : std::to_string(q.mean()).c_str(), root_leaf ? "-" : b.nodes4h.empty() ? "REFUSED" : std::to_string(h.mean()).c_str());
        *report += buf;
    }
    if (!mskbvh::collapse8(b)) { *report += " | 8 REFUSED"; return ""; }
    std::multiset<uint32_t> got; int depth = 0;
    std::string err = walk_wide(b.nodes8, b.root_ref8, 8, &got, &depth);
    if (err.empty() && got != want) err = "the 8-wide tree's leaves are not the binary tree's, each once";
    if (err.empty() && b.max_depth8 < depth) err = "max_depth8 below the walked depth";
    bvhcontain::Stats s8;
    if (err.empty()) err = bvhcontain::check_nodes8(b, &s8);
    if (!err.empty()) return "collapse8: " + err;
    snprintf(buf, sizeof buf, " | 8 depth %d/%d area %.5f", depth, b.max_depth8, s8.mean());
    *report += buf;
    return "";
}
static int run_collapse() {
    int bad = 0;
    for (const CaseSpec &s : all_cases(2049)) {
        Case c; make_case(c, s.family, s.n, s.leaf, s.class_shift);
        if (s.n == 0) continue;
        const Tree t = build(c.in);
        mskbvh::Built twin;
        twin.nodes = t.nodes; twin.tris = t.tris; twin.bounds = t.bounds; twin.root_ref = t.root_ref; twin.max_depth = t.depth;
        std::vector<float> pos((size_t) s.n * 9);
        for (uint32_t k = 0; k < s.n; ++k)
            for (int v = 0; v < 3; ++v)
                for (int a = 0; a < 3; ++a) pos[(size_t) k * 9 + v * 3 + a] = c.verts[(size_t) k * 12 + v * 4 + a];
        mskbvh::Built host = mskbvh::build(pos.data(), s.n, c.in.tri_pad);
        std::string rep_t, rep_h;
        std::string err = check_wide(twin, &rep_t);
        if (!err.empty()) err = "twin tree, " + err;
        else if (!(err = check_wide(host, &rep_h)).empty()) err = "host tree, " + err;
        printf("%s %s: twin%s\n     %*s  host%s%s%s\n", err.empty() ? "ok  " : "FAIL", c.name.c_str(), rep_t.c_str(), (int) c.name.size(), "", rep_h.c_str(), err.empty() ? "" : " — ", err.c_str());
        bad += !err.empty();
    }
    printf(bad ? "FAILED (%d)\n" : "all ok\n", bad);
    return bad ? 1 : 0;
}

static int run_height(const char *path) {
    FILE *f = fopen(path, "rb");
    if (!f) { printf("FAIL cannot open %s\n", path); return 2; }
    uint32_t n = 0; float box[6];
    if (fread(&n, 4, 1, f) != 1 || fread(box, 4, 6, f) != 6) { printf("FAIL short file\n"); return 2; }
    std::vector<float> pos((size_t) n * 9);
    if (fread(pos.data(), 4, pos.size(), f) != pos.size()) { printf("FAIL short file\n"); return 2; }
    fclose(f);
    Case c;
    for (uint32_t k = 0; k < n; ++k) push_tri(c.verts, &pos[(size_t) k * 9]);
    c.finish(2, 0, box, box + 3);
    const Tree t = build(c.in);
    const HostRecords host(c.in);
    Walked w;
    const std::string err = check_tree(c.in, TreeView{t.nodes.data(), t.tris.data(), t.bounds.data(), t.root_ref, t.n_nodes, t.depth}, host, &w);
    if (!err.empty()) { printf("FAIL %s\n", err.c_str()); return 1; }
    printf("ok height %d walked %d nodes %u\n", t.depth, w.depth, t.n_nodes);
    return 0;
}

int main(int argc, char **argv) {
    const std::string mode = argc > 1 ? argv[1] : "twin";
    if (mode == "twin") {
        setenv("MSK_BVH_SWEEP", "0", 0);                  // (the host builder's records, read by prim, do not depend on how it splits)
        return run_twin();
    }
    if (mode == "collapse") return run_collapse();
    if (mode == "height" && argc > 2) return run_height(argv[2]);
    printf("usage: lbvh_tree_check twin | collapse | height <file>\n");
    return 2;
}
