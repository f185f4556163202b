// msk_serial.h — MSK_RNG_PCG_BLOCK on the device: the reference's sampler semantics as written (included by msk_gpu.hip).
//
// samplers/independent.cpp:9-35 gives a render job ONE PCG32 stream per image block (integrator.cpp:56-58 clones the
// sampler per block; SURVEY F7 / oracle D2 fix its seed): a block's samples draw from it in the order the scalar loops
// issue them — y, x, s (integrator.cpp:89-98), and inside a sample: film position (2), wavelength (1), aperture (2),
// then per bounce NEE (2), BSDF lobe (1), BSDF direction (2) and, from rr_depth on, Russian roulette (1)
// (integrator.cpp:103-107, path.cpp:56-73,116-122).  Where a sample's draws start depends on how long every earlier path
// of the block was, so a block is sequential by construction: here ONE LANE renders ONE BLOCK, sample after sample, path
// after path, and splats into the block's bordered buffer with ImageBlock::put's own loops (imageblock.cpp:55-114), in
// order.  Blocks are independent, so a film of B blocks is B lanes wide — a fidelity mode (BASELINE config 1, cbox 256^2
// @ 16 spp, is 64 lanes for three seconds), not a fast one; the wavefront path (MSK_RNG_COUNTER) is the product's hot path.
// The arithmetic of a bounce is the wavefront kernel's (shade_region, msk_kernels.h), call for call — make_interaction,
// bsdf_eval_pdf, bsdf_sample, the emitter sampling of scene.cpp:68-103 — only the control flow is the scalar loop's
// (oracle.cpp: path_sample): a path whose throughput is zero keeps drawing until the loop ends it, as the reference's does,
// because the stream position of the next sample depends on it.  The tree is walked as a binary tree in HBM (traverse<>,
// the arrays every scene has), whatever the scene's trace mode: any tree gives the same hits.
#pragma once

namespace msk {

struct Pcg32 {                                  // core/mathutils.h:85-121
    uint64_t state, inc;
    MSK_DEV uint32_t next_u32() {
        const uint64_t old = state;
        state = old * 0x5851f42d4c957f2dULL + inc;
        const uint32_t xs = (uint32_t) (((old >> 18u) ^ old) >> 27u), rot = (uint32_t) (old >> 59u);
        return (xs >> rot) | (xs << ((~rot + 1u) & 31u));
    }
    MSK_DEV void seed(uint64_t initstate, uint64_t initseq) {
        state = 0u; inc = (initseq << 1u) | 1u;
        next_u32(); state += initstate; next_u32();
    }
    MSK_DEV float next_float() { return u32_to_float01(next_u32()); }
};

struct SerialParams {
    uint64_t seed;
    uint32_t spp, sample_first, sample_stride;
    int32_t rr_depth, max_depth, hide_emitters;
    const BlockInfo *blocks; uint32_t n_blocks;
    float *block_buf; uint32_t buf_stride;
    uint32_t *stack_ovf;
    uint32_t per_wave;          // 1: image block = wave index, only lane 0 works (see k_path_serial)
    unsigned long long *counters;               // [0] samples [1] segments [2] shadow rays [3] invalid samples (imageblock.cpp:57-81)
};

// ImageBlock::put(pos, value) (imageblock.cpp:55-114) into a bordered block buffer of sx x sy pixels, 5 channels
MSK_DEV void serial_put(const DeviceScene &sc, float *data, int sx, int sy, int org_x, int org_y, float pos_x, float pos_y, const float (&value)[5]) {
    const float radius = sc.filter_radius;
    const float px = pos_x - 0.5f - (float) org_x, py = pos_y - 0.5f - (float) org_y;       // org = offset - border
    const int lo_x = max((int) ceilf(px - radius), 0), lo_y = max((int) ceilf(py - radius), 0);
    const int hi_x = min((int) floorf(px + radius), sx - 1), hi_y = min((int) floorf(py + radius), sy - 1);
    for (int y = lo_y; y <= hi_y; ++y) {
        const float wy = sc.lut[min((int) fabsf(((float) y - py) * sc.filter_scale), MSK_FILTER_RESOLUTION)];      // rfilter.h:13-16
        for (int x = lo_x; x <= hi_x; ++x) {
            const float wx = sc.lut[min((int) fabsf(((float) x - px) * sc.filter_scale), MSK_FILTER_RESOLUTION)];
            const float weight = wx * wy;
            float *dest = data + ((size_t) y * sx + x) * 5;
#pragma unroll
            for (int k = 0; k < 5; ++k) dest[k] += weight * value[k];
        }
    }
}

// The kernel's body lives in msk_serial_body.inc and is included into each kernel: TB = SceneTablesR, or SceneTablesD for a scene
// that holds a smooth `dielectric` (k_path_serial_d), which alone compiles the guard around next-event estimation.
// One kernel per family of MSK_FAMILIES (msk_kernels.h) whose SERIAL field says YES, written by hand: an #include cannot be stamped from
// a list, and through a function over TB the compiler lays all six out differently (EXPERIMENTS.md, "Name each shading family once").
__global__ void __launch_bounds__(MSK_BLOCK)
k_path_serial(DeviceScene sc, SerialParams prm) {
    typedef SceneTablesR TB;
#include "msk_serial_body.inc"
}
__global__ void __launch_bounds__(MSK_BLOCK)
k_path_serial_d(DeviceScene sc, SerialParams prm) {
    typedef SceneTablesD TB;
#include "msk_serial_body.inc"
}
// ... and SceneTablesB for a scene that holds a `bitmap` texture (with or without glass)
__global__ void __launch_bounds__(MSK_BLOCK)
k_path_serial_b(DeviceScene sc, SerialParams prm) {
    typedef SceneTablesB TB;
#include "msk_serial_body.inc"
}
// ... and SceneTablesE for a scene whose environment emitter is an image (whatever else it holds)
__global__ void __launch_bounds__(MSK_BLOCK)
k_path_serial_e(DeviceScene sc, SerialParams prm) {
    typedef SceneTablesE TB;
#include "msk_serial_body.inc"
}
// ... and SceneTablesP for a scene that holds a `point` emitter or a smooth `conductor` (whatever else it holds)
__global__ void __launch_bounds__(MSK_BLOCK)
k_path_serial_p(DeviceScene sc, SerialParams prm) {
    typedef SceneTablesP TB;
#include "msk_serial_body.inc"
}
// ... and SceneTablesM for a scene that holds a `mask` (whatever else it holds)
__global__ void __launch_bounds__(MSK_BLOCK)
k_path_serial_m(DeviceScene sc, SerialParams prm) {
    typedef SceneTablesM TB;
#include "msk_serial_body.inc"
}

}  // namespace msk
