// msk_lens.h — the camera ray, for the pinhole and for the `thinlens` sensor (include/msk_gpu.h: msk_camera_desc, msk_lens_desc).
// ONE function: shade_region's regeneration, k_direct and the probe k_camera_probe call it.  LENS is a compile-time choice: with
// LENS = false the function is the pinhole's arithmetic exactly as its three callers used to spell it (PerspectiveCamera::sample_ray,
// perspective.cpp:22-42; Transform4f::apply_point / apply_vector), expression for expression, so the instantiations every scene
// without a lens runs keep their code; with LENS = true it is the six steps of msk_lens_desc.
#pragma once

namespace msk {

struct CameraRay { f3 o, d; float tnear, tfar; };

// s2c, to_world: row-major 4x4 (DeviceScene, or the regeneration's copies of them); (px, py): the film position in pixels;
// u: the aperture sample, lens_radius, focus_distance: read only where LENS
template <bool LENS>
MSK_DEV CameraRay camera_ray(const float *s2c, const float *to_world, float near_clip, float far_clip, float lens_radius, float focus_distance,
                             float px, float py, f2 u) {
    CameraRay r;
    float r4[4];
#pragma unroll
    for (int q4 = 0; q4 < 4; ++q4)
        r4[q4] = ((s2c[q4 * 4 + 0] * px + s2c[q4 * 4 + 1] * py) + s2c[q4 * 4 + 2] * 0.f) + s2c[q4 * 4 + 3] * 1.f;
    const f3 near_p = mk3(r4[0] / r4[3], r4[1] / r4[3], r4[2] / r4[3]);
    float lx = 0.f, ly = 0.f;
    f3 dl;
    if (LENS) {
        const f2 a = square_to_uniform_disk_concentric(u);
        lx = a.x * lens_radius; ly = a.y * lens_radius;
        const float ft = focus_distance / near_p.z;
        const f3 fp = mk3(near_p.x * ft, near_p.y * ft, near_p.z * ft);
        dl = normalized(mk3(fp.x - lx, fp.y - ly, fp.z));
    } else dl = normalized(near_p);
    const float inv_z = 1.f / dl.z;
    float o4[4];
#pragma unroll
    for (int q4 = 0; q4 < 4; ++q4)
        o4[q4] = ((to_world[q4 * 4 + 0] * lx + to_world[q4 * 4 + 1] * ly) + to_world[q4 * 4 + 2] * 0.f) +
                 to_world[q4 * 4 + 3] * 1.f;
    r.o = mk3(o4[0] / o4[3], o4[1] / o4[3], o4[2] / o4[3]);
    const float *m = to_world;
    r.d = mk3(m[0] * dl.x + (m[1] * dl.y + m[2] * dl.z), m[4] * dl.x + (m[5] * dl.y + m[6] * dl.z),
              m[8] * dl.x + (m[9] * dl.y + m[10] * dl.z));
    r.tnear = near_clip * inv_z; r.tfar = far_clip * inv_z;
    return r;
}

}  // namespace msk
