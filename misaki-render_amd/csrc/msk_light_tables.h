// msk_light_tables.h — the `spot` / `directional` part of msk_scene_tables.h (include/msk_gpu.h: msk_light_desc): the refusals of the
// descriptors and the two records' layout (msk_layout.h: MSK_EMITTER_MARK_SPOT / _DIRECTIONAL).  Plain C++17, no HIP;
// tests/native/light_tables_check.cpp checks every refusal and every packed byte on a CPU.
// The emitter record stays two float4.  A sun: {c0, c1, c2, 0} {MARK_DIRECTIONAL, d} with d = -direction, the way TO the light.  A
// spot: {c0, c1, c2, offset (uint bits)} {MARK_SPOT, position}; its five floats {axis, cos_cutoff, cos_beam} lie in the pool that
// holds the area emitters' CDFs, at that offset: a delta light has no area density in word 3.  A scene without the two types gets
// neither record nor pool entry: its tables are what they were.
#pragma once
#include "msk_layout.h"
#include "../../include/msk_gpu.h"

#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

namespace mskscene {

// the text of a refusal, as msk_gpu.hip's fail_to writes it
inline int refuse_light(std::string *msg, int code, const char *fmt, ...) {
    char buf[1024];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
    *msg = buf;
    return code;
}

inline int check_light_list(uint32_t n_lights, const msk_light_desc *lights, std::string *msg) {
    if (n_lights && !lights) return refuse_light(msg, MSK_ERR_INVALID_ARG, "msk_scene_lights: n_lights %u without lights", n_lights);
    return MSK_OK;
}

// every descriptor names a spot or directional emitter of the scene (after the emitters' own loop: a scene's first fault is an emitter's)
inline int check_light_emitters(const msk_scene_desc *d, uint32_t n_lights, const msk_light_desc *lights, std::string *msg) {
    for (uint32_t k = 0; k < n_lights; ++k) {
        const uint32_t le = lights[k].emitter;
        if (le >= d->n_emitters) return refuse_light(msg, MSK_ERR_INVALID_ARG, "msk_light_desc %u: emitter %u out of range (the scene has %u)", k, le, d->n_emitters);
        if (d->emitters[le].type != MSK_EMITTER_SPOT && d->emitters[le].type != MSK_EMITTER_DIRECTIONAL)
            return refuse_light(msg, MSK_ERR_INVALID_ARG, "msk_light_desc %u: emitter %u is of type %d, neither a spot (type %d) nor a directional emitter (type %d)", k, le,
                                d->emitters[le].type, MSK_EMITTER_SPOT, MSK_EMITTER_DIRECTIONAL);
    }
    return MSK_OK;
}

// the record of emitter e, a spot or a directional emitter, into o[0 .. 8) (o[0 .. 3) hold its spectrum's coefficients already)
inline int pack_light_record(uint32_t e, const msk_emitter_desc &ed, uint32_t n_lights, const msk_light_desc *lights, float *o, std::vector<float> &cdf_all, bool &has_delta,
                             bool &has_directional, std::string *msg) {
    const bool spot = ed.type == MSK_EMITTER_SPOT;
    const char *what = spot ? "spot" : "directional";
    if (ed.mesh_id != -1) return refuse_light(msg, MSK_ERR_INVALID_ARG, "emitter %u: a %s emitter has no mesh (mesh_id must be -1)", e, what);
    const msk_light_desc *ld = nullptr;
    for (uint32_t k = 0; k < n_lights; ++k)
        if (lights[k].emitter == e) {
            if (ld) return refuse_light(msg, MSK_ERR_INVALID_ARG, "emitter %u: a %s emitter with two descriptors (msk_light_desc %u is its second)", e, what, k);
            ld = &lights[k];
        }
    if (!ld) return refuse_light(msg, MSK_ERR_INVALID_ARG, "emitter %u: a %s emitter needs its geometry (msk_gpu_scene_create_lights with an msk_light_desc)", e, what);
    if (spot && (!std::isfinite(ld->position[0]) || !std::isfinite(ld->position[1]) || !std::isfinite(ld->position[2])))
        return refuse_light(msg, MSK_ERR_INVALID_ARG, "emitter %u: a spot emitter's position must be finite", e);
    if (!std::isfinite(ld->direction[0]) || !std::isfinite(ld->direction[1]) || !std::isfinite(ld->direction[2]))
        return refuse_light(msg, MSK_ERR_INVALID_ARG, "emitter %u: a %s emitter's direction must be finite", e, what);
    const float n2 = ld->direction[0] * ld->direction[0] + (ld->direction[1] * ld->direction[1] + ld->direction[2] * ld->direction[2]);
    if (!(std::fabs(n2 - 1.f) <= 1e-5f))
        return refuse_light(msg, MSK_ERR_INVALID_ARG, "emitter %u: a %s emitter's direction must have unit length (its squared length is %.9g)", e, what, (double) n2);
    has_delta = true;
    o[3] = 0.f;
    if (!spot) {
        has_directional = true;
        const uint32_t mark = MSK_EMITTER_MARK_DIRECTIONAL;
        const float dir[3] = {-ld->direction[0], -ld->direction[1], -ld->direction[2]};       // the way TO the light
        std::memcpy(&o[4], &mark, 4); std::memcpy(&o[5], dir, 12);
        return MSK_OK;
    }
    if (!(ld->cos_cutoff >= -1.f && ld->cos_cutoff < 1.f))
        return refuse_light(msg, MSK_ERR_INVALID_ARG, "emitter %u: a spot emitter's cos_cutoff %.9g is outside [-1, 1)", e, (double) ld->cos_cutoff);
    if (!(ld->cos_beam >= ld->cos_cutoff && ld->cos_beam <= 1.f))
        return refuse_light(msg, MSK_ERR_INVALID_ARG, "emitter %u: a spot emitter's cos_beam %.9g is outside [cos_cutoff, 1] (cos_cutoff %.9g)", e, (double) ld->cos_beam,
                            (double) ld->cos_cutoff);
    const uint32_t mark = MSK_EMITTER_MARK_SPOT, off = (uint32_t) cdf_all.size();
    std::memcpy(&o[3], &off, 4);
    std::memcpy(&o[4], &mark, 4); std::memcpy(&o[5], ld->position, 12);
    cdf_all.insert(cdf_all.end(), ld->direction, ld->direction + 3);
    cdf_all.push_back(ld->cos_cutoff); cdf_all.push_back(ld->cos_beam);
    return MSK_OK;
}

}  // namespace mskscene
