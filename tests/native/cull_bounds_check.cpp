// The bounds of the camera cull (msk_bvh.h: cull_bounds — what msk_gpu_scene_create puts into DeviceScene::cull_lo / cull_hi),
// compiled and run by tests/test_camera_cull.py.  Builds the host's binary tree over the triangles of a file and prints what the
// test compares: the root's record as the tree stores it, and the bounds taken from it.
// usage: cull_bounds_check <file of 9 float32 per triangle> <tri_pad>
// prints: "tris N root_ref R on B" / "node f0 .. f11" (hex floats; only when the root is an inner node) / "lo x y z" / "hi x y z"
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../misaki-render_amd/csrc/msk_bvh.h"

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    std::vector<float> pos;
    if (FILE *f = std::fopen(argv[1], "rb")) {
        float buf[9];
        while (std::fread(buf, sizeof(float), 9, f) == 9) pos.insert(pos.end(), buf, buf + 9);
        std::fclose(f);
    } else return 2;
    const uint32_t n = (uint32_t) (pos.size() / 9);
    const mskbvh::Built b = mskbvh::build(pos.data(), n, (float) std::atof(argv[2]));
    const mskbvh::CullBounds c = mskbvh::cull_bounds(b.nodes, b.root_ref, n);
    std::printf("tris %u root_ref %u on %d\n", n, b.root_ref, c.on ? 1 : 0);
    if (n && !(b.root_ref & 0x80000000u)) {
        std::printf("node");
        for (int k = 0; k < 12; ++k) std::printf(" %a", b.nodes[(size_t) b.root_ref * 16 + k]);
        std::printf("\n");
    }
    std::printf("lo %a %a %a\nhi %a %a %a\n", c.lo[0], c.lo[1], c.lo[2], c.hi[0], c.hi[1], c.hi[2]);
    return 0;
}
