// direct_plan_probe.cpp — which k_direct a scene gets, on a CPU, for tests/test_direct_oracle_parity.py: the host side of
// msk_gpu_scene_create (csrc/msk_scene_tables.h: pack; csrc/msk_bvh.h: build and the collapses; csrc/msk_plan.h: place_tree,
// place_tables) followed by make_direct_plan, with the knobs read from the environment as the library reads them.  Built as a shared
// library and called through ctypes with the msk_scene_desc a test hands to the library.  (MSK_BVH_BUILD=gpu builds the tree on the
// device: the host builder's tree stands in for its node count and depth here, which the form and tables_mode of these scenes do not
// hang on — the test that uses it says so.)
#include "../../misaki-render_amd/csrc/msk_scene_tables.h"
#include "../../misaki-render_amd/csrc/msk_bvh.h"
#include "../../misaki-render_amd/csrc/msk_plan.h"

#include <cstdio>
#include <string>

// out[0] form (k_direct's MODE: 0, 6 or 1), [1] tables_mode, [2] the scene's trace mode, [3] stack entries in LDS, [4] overflow entries,
// [5] LDS bytes of a block, [6] binary-tree nodes, [7] binary-tree depth, [8] bytes the scene's own placement stages, [9] records per wave
extern "C" int direct_plan_probe(const msk_scene_desc *d, const msk_scene_masks *em, uint32_t light_samples, uint32_t bsdf_samples,
                                 uint64_t pass_records, int64_t *out, char *msg_out, int msg_len) {
    const msk_scene_ext *ext = em ? &em->ext : nullptr;
    const mskplan::SceneKnobs knobs = mskplan::read_scene_knobs();
    mskscene::HostTables t;
    std::string msg;
    if (int rc = mskscene::pack(d, ext, knobs.pad_scale, &t, &msg, em ? em->n_masks : 0u, em ? em->masks : nullptr)) {
        std::snprintf(msg_out, (size_t) msg_len, "%s", msg.c_str());
        return rc;
    }
    mskbvh::Built bvh = mskbvh::build(t.pos.data(), d->n_faces, t.tri_pad);
    mskplan::BinaryTree binary;
    binary.n_nodes = (uint32_t) (bvh.nodes.size() / 16); binary.n_tris = d->n_faces; binary.max_depth = bvh.max_depth;
    binary.root_is_leaf = (bvh.root_ref & MSK_LEAF_BIT) != 0;
    const mskplan::TreePlacement tree = mskplan::place_tree(binary, knobs, [&](int width) {
        mskplan::WideTree w;
        if (width == 8) { w.ok = mskbvh::collapse8(bvh); w.max_depth = bvh.max_depth8; w.n_nodes = (uint32_t) (bvh.nodes8.size() / 32); }
        else {
            mskbvh::collapse4(bvh, knobs.collapse_optimal);
            w.ok = true; w.max_depth = bvh.max_depth4; w.n_nodes = (uint32_t) (bvh.nodes4.size() / 32); w.has_half = !bvh.nodes4h.empty(); w.has_byte = !bvh.nodes4q.empty();
        }
        return w;
    });
    mskplan::TableCounts counts;
    counts.n_tris = d->n_faces; counts.n_meshes = d->n_meshes; counts.n_bsdf_f4 = t.n_bsdf_f4; counts.n_emitters = d->n_emitters;
    counts.cdf_len = (uint32_t) t.cdf_all.size(); counts.n_spectra = d->n_regular_values;
    const mskplan::TablePlacement tables = mskplan::place_tables(counts);
    mskplan::SceneFacts f;
    f.trace_mode = tree.trace_mode; f.lds_scene = tree.lds_scene; f.trace_lds_bytes = tree.trace_lds_bytes;
    f.lds_tables = tables.lds_tables; f.shade_lds_bytes = tables.shade_lds_bytes;
    const mskplan::DirectPlan p = mskplan::make_direct_plan(f, tree.stack_entries, tree.stack_total, bvh.max_depth, light_samples, bsdf_samples, pass_records);
    out[0] = p.form; out[1] = p.tables_mode; out[2] = tree.trace_mode; out[3] = p.stack_entries; out[4] = p.ovf_entries;
    out[5] = (int64_t) p.lds_bytes; out[6] = binary.n_nodes; out[7] = bvh.max_depth; out[8] = (int64_t) tables.staged_bytes; out[9] = p.records_per_wave;
    return 0;
}
