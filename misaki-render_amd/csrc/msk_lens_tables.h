// msk_lens_tables.h — the host side of the `thinlens` sensor (include/msk_gpu.h: msk_lens_desc): the refusals of the descriptor, and
// what a scene with a lens needs of the tables.  Plain C++17, no HIP; tests/native/lens_check.cpp checks every refusal on a CPU.
// A scene with a lens runs the SceneTablesL instantiations (msk_kernels.h), which carry the mask code: such a scene must have the
// mask records at the end of `bsdfs`.  One that holds no mask gets them here, every entry the constant opacity 1 — the record
// pack_mask_records (msk_mask_tables.h) writes for an entry without a mask — under which the mask code is the nested BSDF to the bit.
#pragma once
#include "msk_scene_tables.h"

#include <cmath>
#include <string>

namespace mskscene {

// MSK_OK, or MSK_ERR_INVALID_ARG with a text that names the field
inline int check_lens(const msk_lens_desc *lens, std::string *msg) {
    if (!lens) return MSK_OK;
    if (!(std::isfinite(lens->aperture_radius) && lens->aperture_radius >= 0.f))
        return refuse(msg, MSK_ERR_INVALID_ARG, "msk_lens_desc: aperture_radius %.9g must be finite and not negative", (double) lens->aperture_radius);
    if (!(std::isfinite(lens->focus_distance) && lens->focus_distance > 0.f))
        return refuse(msg, MSK_ERR_INVALID_ARG, "msk_lens_desc: focus_distance %.9g must be finite and greater than 0", (double) lens->focus_distance);
    return MSK_OK;
}

// the tables of a scene with a lens, from those pack() made for the same scene without one
inline void add_lens_tables(const msk_scene_desc *d, HostTables *t) {
    t->all_diffuse = false;          // the lens kernels are instantiations of the general shading variant
    if (t->has_mask || t->has_plastic) return;         // the records are there
    add_unit_mask_records(d->n_bsdfs, t->bsdfs, t->n_bsdf_f4, t->mask_base);      // {filter 0 = constant, opacity 1} (msk_plastic_tables.h)
}

}  // namespace mskscene
