// GPU side of tests/test_lbvh_tree.py: msklbvh::build (msk_lbvh.hip, included as tools/micro/lbvh_sort_test.hip includes it)
// against its scalar CPU twin (lbvh_ref.h), bit for bit, on every input of lbvh_ref.h.  Per case: the builder writes into buffers
// filled with a sentinel word, with guard records behind the n node, triangle and bounds records; root_ref, n_nodes, depth, the
// first n_nodes nodes, the triangles and the bounds equal the twin's; the checks that do not rest on the twin pass on the
// device's output itself; everything behind n_nodes nodes and the guards still holds the sentinel; a second build of the same
// input gives the same bytes (k_refit's arrival order must not matter).  Prints one line per case and "all ok".  The first HIP
// error is printed and ends the program, non-zero, before another build is started.
#include "../../misaki-render_amd/csrc/msk_lbvh.hip"
#include "lbvh_ref.h"
#include <cstdio>
#include <cstdlib>
#include <vector>

#define HIP_OK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error: %s: %s\n", #x, hipGetErrorString(e_)); fflush(stdout); exit(3); } } while (0)

static constexpr uint32_t kGuard = 64;                    // records behind the n the builder may write
static constexpr uint32_t kSentinel = 0xa5a5a5a5u;

struct Out { std::vector<uint32_t> nodes, tris, bounds; msklbvh::Result res; };

static bool all_sentinel(const std::vector<uint32_t> &v, size_t from) {
    for (size_t k = from; k < v.size(); ++k) if (v[k] != kSentinel) return false;
    return true;
}

int main() {
    using namespace lbvhref;
    setenv("MSK_BVH_SWEEP", "0", 0);                      // (the host builder's records, read by prim, do not depend on how it splits)
    const std::vector<CaseSpec> cases = all_cases();
    uint32_t max_n = 0;
    for (const CaseSpec &s : cases) max_n = std::max(max_n, s.n);
    const size_t cap = (size_t) max_n + kGuard;
    float4 *d_verts, *d_nodes, *d_tris, *d_bounds, *d_bsdfs; int4 *d_mesh;
    HIP_OK(hipMalloc(&d_verts, std::max<size_t>(max_n, 1) * 48)); HIP_OK(hipMalloc(&d_nodes, cap * 64)); HIP_OK(hipMalloc(&d_tris, cap * 64));
    HIP_OK(hipMalloc(&d_bounds, cap * 32)); HIP_OK(hipMalloc(&d_bsdfs, 4 * MSK_BSDF_F4 * 16)); HIP_OK(hipMalloc(&d_mesh, 6 * 16));
    int bad = 0;
    for (const CaseSpec &s : cases) {
        Case c; make_case(c, s.family, s.n, s.leaf, s.class_shift);
        const uint32_t n = s.n;
        const Tree twin = build(c.in);
        const HostRecords host(c.in);
        if (n) HIP_OK(hipMemcpy(d_verts, c.verts.data(), (size_t) n * 48, hipMemcpyHostToDevice));
        HIP_OK(hipMemcpy(d_mesh, c.mesh_info.data(), 6 * 16, hipMemcpyHostToDevice));
        HIP_OK(hipMemcpy(d_bsdfs, c.bsdfs.data(), c.bsdfs.size() * 4, hipMemcpyHostToDevice));
        msklbvh::Input in;
        in.tri_verts = n ? d_verts : nullptr; in.n_tris = n;
        for (int a = 0; a < 3; ++a) { in.lo[a] = c.in.lo[a]; in.hi[a] = c.in.hi[a]; }
        in.box_pad = c.in.box_pad; in.tri_pad = c.in.tri_pad; in.leaf_size = c.in.leaf_size;
        in.mesh_info = d_mesh; in.bsdfs = d_bsdfs; in.n_bsdfs = c.in.n_bsdfs; in.bsdf_f4 = c.in.bsdf_f4; in.class_shift = c.in.class_shift;
        const size_t recs = (size_t) n + kGuard;
        Out o[2];
        for (int pass = 0; pass < 2; ++pass) {             // two builds of the same input, not a loop over attempts
            HIP_OK(hipMemset(d_nodes, 0xa5, recs * 64)); HIP_OK(hipMemset(d_tris, 0xa5, recs * 64)); HIP_OK(hipMemset(d_bounds, 0xa5, recs * 32));
            HIP_OK(hipDeviceSynchronize());
            char err[256] = "";
            if (msklbvh::build(nullptr, in, d_nodes, d_tris, d_bounds, &o[pass].res, err, sizeof err)) { printf("HIP error in build: %s\n", err); fflush(stdout); return 3; }
            HIP_OK(hipDeviceSynchronize());
            o[pass].nodes.resize(recs * 16); o[pass].tris.resize(recs * 16); o[pass].bounds.resize(recs * 8);
            HIP_OK(hipMemcpy(o[pass].nodes.data(), d_nodes, recs * 64, hipMemcpyDeviceToHost));
            HIP_OK(hipMemcpy(o[pass].tris.data(), d_tris, recs * 64, hipMemcpyDeviceToHost));
            HIP_OK(hipMemcpy(o[pass].bounds.data(), d_bounds, recs * 32, hipMemcpyDeviceToHost));
        }
        const Out &g = o[0];
        std::string e;
        Walked w;
        if (g.res.root_ref != twin.root_ref || g.res.n_nodes != twin.n_nodes || g.res.depth != twin.depth) {
            char m[160]; snprintf(m, sizeof m, "root %#x nodes %u depth %d, the twin has root %#x nodes %u depth %d", g.res.root_ref, g.res.n_nodes, g.res.depth, twin.root_ref, twin.n_nodes, twin.depth);
            e = m;
        }
        else if (g.res.n_nodes > n) e = "more nodes than triangles";
        else if (g.res.n_nodes && memcmp(g.nodes.data(), twin.nodes.data(), (size_t) g.res.n_nodes * 64)) {
            size_t k = 0; while (g.nodes[k] == f2u(twin.nodes[k])) ++k;
            char m[160]; snprintf(m, sizeof m, "node %zu word %zu: %#x, the twin has %#x", k / 16, k % 16, g.nodes[k], f2u(twin.nodes[k]));
            e = m;
        }
        else if (n && memcmp(g.tris.data(), twin.tris.data(), (size_t) n * 64)) e = "triangle records differ from the twin's";
        else if (n && memcmp(g.bounds.data(), twin.bounds.data(), (size_t) n * 32)) e = "bounds differ from the twin's";
        if (e.empty())
            e = check_tree(c.in, TreeView{(const float *) g.nodes.data(), (const float *) g.tris.data(), (const float *) g.bounds.data(), g.res.root_ref, g.res.n_nodes, g.res.depth}, host, &w);
        if (e.empty() && !all_sentinel(g.nodes, (size_t) g.res.n_nodes * 16)) e = "a write behind the n_nodes node records";
        if (e.empty() && (!all_sentinel(g.tris, (size_t) n * 16) || !all_sentinel(g.bounds, (size_t) n * 8))) e = "a write behind the n triangle records or bounds";
        if (e.empty() && (o[1].res.root_ref != g.res.root_ref || o[1].res.n_nodes != g.res.n_nodes || o[1].res.depth != g.res.depth || o[1].nodes != g.nodes || o[1].tris != g.tris || o[1].bounds != g.bounds))
            e = "a second build of the same input differs";
        printf("%s %s: depth %d walked %d nodes %u leaves %u%s%s\n", e.empty() ? "ok  " : "FAIL", c.name.c_str(), g.res.depth, w.depth, g.res.n_nodes, w.leaves, e.empty() ? "" : " — ", e.c_str());
        bad += !e.empty();
    }
    HIP_OK(hipFree(d_verts)); HIP_OK(hipFree(d_nodes)); HIP_OK(hipFree(d_tris)); HIP_OK(hipFree(d_bounds)); HIP_OK(hipFree(d_bsdfs)); HIP_OK(hipFree(d_mesh));
    printf(bad ? "FAILED (%d)\n" : "all ok\n", bad);
    return bad ? 1 : 0;
}
