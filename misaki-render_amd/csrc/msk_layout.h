// msk_layout.h — the constants of the device data layout that host code needs too: the table packer (msk_scene_tables.h) and the
// placement (msk_plan.h) read them on a CPU, msk_device.h and msk_kernels.h include this file for the kernels.  Preprocessor
// constants only, no HIP, no C++: each value is written here and nowhere else.
#pragma once

#define MSK_WAVE 64
#define MSK_BLOCK 256
#define MSK_BSDF_F4 7   /* float4 per BSDF record (built from msk_bsdf_desc by mskscene::pack, msk_scene_tables.h) */
#define MSK_LEAF_BIT 0x80000000u  /* child ref: leaf = BIT | first_tri << 5 | count ; inner = node index */
/* bits 27..28 of a triangle record's / hit record's prim word: the MATERIAL CLASS of the triangle's BSDF (msk_kernels.h, at MSK_PRIM_ID) */
#define MSK_CLASS_SHIFT 27
#define MSK_N_CLASSES 4
#define MSK_EMITTER_MARK_POINT 0xfffffffeu      /* word 0 of a point emitter's second float4 (an environment emitter's: 0xffffffff) */
/* the other delta lights (msk_gpu.h, msk_light_desc).  A spot: {MARK_SPOT, position}; word 3 of its FIRST float4 holds, as bits,
   the offset in the CDF pool of its five floats {axis.x, axis.y, axis.z, cos_cutoff, cos_beam}.  A sun: {MARK_DIRECTIONAL, d} with
   d = -direction, the way to the light.  The three marks are consecutive: MSK_EMITTER_MARK_DELTA_FIRST <= mark <= MARK_POINT. */
#define MSK_EMITTER_MARK_SPOT 0xfffffffdu
#define MSK_EMITTER_MARK_DIRECTIONAL 0xfffffffcu
#define MSK_EMITTER_MARK_DELTA_FIRST MSK_EMITTER_MARK_DIRECTIONAL

/* core/mathutils.h:10-20 */
#define MSK_EPSILON_F   5.9604644775390625e-08f
#define MSK_RAY_EPS_F   (MSK_EPSILON_F * 1500)

/* the done-queues of k_shade_gen (msk_kernels.h, DoneQueue) */
#define MSK_DONE_Q 128                     /* entries per wave: up to 63 parked + 64 new */
#define MSK_DONE_Q_F4 (MSK_DONE_Q * 5 / 2)  /* float4 of LDS per wave: wl and res (16 B per entry), id (8 B) */

/* the small shading tables are staged in LDS up to this size (msk_kernels.h: stage_tables; compile time, 0 = never) */
#ifndef MSK_SMALL_TABLES_KB
#define MSK_SMALL_TABLES_KB 16
#endif
