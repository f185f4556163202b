// Host-side check of msk_bvh.h's quantised 4-wide nodes (Built::nodes4q), compiled and run by tests/test_bvh_host.py:
// every decoded child box must contain the padded full-precision box of nodes4 (the traversal only ever culls), the grid must be
// the finest that spans the node (area growth of a per cent or so), unused slots must be inverted boxes pointing at an empty leaf.
// (The containment loops live in bvh_contain.h, which lbvh_tree_check.cpp runs on the device builder's trees as well.)
// usage: bvh_quant_check <n_triangles> <seed> <scale>     prints "ok ..." or "FAIL ..."
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>
#include "bvh_contain.h"

int main(int argc, char **argv) {
    const uint32_t n = argc > 1 ? (uint32_t) atoi(argv[1]) : 20000;
    const uint32_t seed = argc > 2 ? (uint32_t) atoi(argv[2]) : 1;
    const float world = argc > 3 ? (float) atof(argv[3]) : 1.f;
    std::mt19937 rng(seed);
    std::uniform_real_distribution<float> u(-1.f, 1.f);
    std::vector<float> pos((size_t) n * 9);
    for (uint32_t t = 0; t < n; ++t) {
        float c[3] = {u(rng) * 300.f, u(rng) * 300.f, u(rng) * 300.f};
        const float size = std::pow(10.f, u(rng) * 1.2f);                     // sizes over more than two decades
        const int kind = (int) (rng() % 10);
        for (int v = 0; v < 3; ++v)
            for (int a = 0; a < 3; ++a) {
                float d = u(rng) * size;
                if (kind == 0 && a == (int) (t % 3)) d = 0.f;                 // axis-aligned triangles: a degenerate box axis
                if (kind == 1 && v == 2) d *= 1e-4f;                          // slivers
                pos[(size_t) t * 9 + v * 3 + a] = (c[a] + d) * world;
            }
    }
    mskbvh::Built b = mskbvh::build(pos.data(), n, 0.05f * world);
    mskbvh::collapse4(b);
    const size_t nn = b.nodes4.size() / 32;
    bvhcontain::Stats q, h;                        // the byte grid (nodes4q); the half-float twin (nodes4h, 80-byte nodes): same containment
    std::string err = bvhcontain::check_nodes4q(b, &q);
    if (err.empty()) err = bvhcontain::check_nodes4h(b, &h);
    if (!err.empty()) { printf("FAIL %s\n", err.c_str()); return 1; }
    const double area_ratio = q.area_ratio, area_ratio_h = h.area_ratio; const size_t children = q.children, children_h = h.children, empty = q.empty;
    printf("ok half_area_ratio %.5f nodes %zu children %zu unused_slots %zu mean_area_ratio %.5f depth4 %d\n", children_h ? area_ratio_h / children_h : 1.0, nn, children, empty, children ? area_ratio / children : 1.0, b.max_depth4);
    return 0;
}
