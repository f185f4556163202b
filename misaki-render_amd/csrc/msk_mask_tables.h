// msk_mask_tables.h — the `mask` part of msk_scene_tables.h (include/msk_gpu.h: msk_mask_desc): the refusals of the descriptors and the
// mask records' layout.  Plain C++17, no HIP; tests/native/mask_tables_check.cpp checks every refusal and every packed byte on a CPU.
// In a scene that holds a mask EVERY BSDF entry has a mask record, three float4 at the end of the BSDF table (entry b: float4
// mask_base + 3 b; msk_kernels.h: mask_record, mask_opacity): {first value (index into `texels` read as floats), W, H (uint bits), m02}
// {filter (uint bits), opacity, 0, m12} {m00 m01 m10 m11}; an entry without a mask: the constant 1.  The images' values lie behind
// everything else in the texel pool, one float each, padded to a float4.  A scene without masks gets neither.
#pragma once
#include "../../include/msk_gpu.h"

#include <algorithm>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

namespace mskscene {

// the text of a refusal, as msk_gpu.hip's fail_to writes it
inline int refuse_mask(std::string *msg, int code, const char *fmt, ...) {
    char buf[1024];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
    *msg = buf;
    return code;
}

inline int pack_mask_records(const msk_scene_desc *d, uint32_t n_masks, const msk_mask_desc *masks, std::vector<float> &bsdfs, uint32_t &n_bsdf_f4, bool &has_mask,
                             bool &has_mask_image, uint32_t &mask_base, std::vector<float> &mask_values, std::string *msg) {
    if (n_masks == 0) return MSK_OK;
    if (!masks) return refuse_mask(msg, MSK_ERR_INVALID_ARG, "msk_scene_masks: n_masks %u without masks", n_masks);
    std::vector<int> seen(std::max(1u, d->n_bsdfs), -1);
    for (uint32_t k = 0; k < n_masks; ++k) {
        const msk_mask_desc &m = masks[k];
        if (m.bsdf >= d->n_bsdfs) return refuse_mask(msg, MSK_ERR_INVALID_ARG, "mask %u: bsdf %u out of range (the scene has %u)", k, m.bsdf, d->n_bsdfs);
        if (seen[m.bsdf] >= 0) return refuse_mask(msg, MSK_ERR_INVALID_ARG, "mask %u: bsdf %u already has a mask (mask %d): at most one per entry", k, m.bsdf, seen[m.bsdf]);
        seen[m.bsdf] = (int) k;
        if (m.filter < 0 || m.filter > 2) return refuse_mask(msg, MSK_ERR_INVALID_ARG, "mask %u: filter %d is not 0 (constant), 1 (nearest) or 2 (bilinear)", k, m.filter);
        if (m.filter == 0) {
            if (!(m.opacity >= 0.f && m.opacity <= 1.f)) return refuse_mask(msg, MSK_ERR_INVALID_ARG, "mask %u: the opacity %g is not in [0, 1]", k, (double) m.opacity);
            continue;
        }
        if (m.width < 1 || m.height < 1) return refuse_mask(msg, MSK_ERR_INVALID_ARG, "mask %u: an image of %u x %u values (width and height must be at least 1)", k, m.width, m.height);
        if (!m.values) return refuse_mask(msg, MSK_ERR_INVALID_ARG, "mask %u: an image, but its values array is missing", k);
        if ((uint64_t) m.width * m.height >= (1ull << 28)) return refuse_mask(msg, MSK_ERR_UNSUPPORTED, "mask %u: %u x %u values, this back end takes fewer than 2^28", k, m.width, m.height);
        const size_t n = (size_t) m.width * m.height;
        for (size_t i = 0; i < n; ++i)
            if (!(m.values[i] >= 0.f && m.values[i] <= 1.f)) return refuse_mask(msg, MSK_ERR_INVALID_ARG, "mask %u: value %zu, %g, is not in [0, 1]", k, i, (double) m.values[i]);
    }
    has_mask = true;
    mask_base = n_bsdf_f4;
    n_bsdf_f4 += 3u * d->n_bsdfs;
    bsdfs.resize((size_t) n_bsdf_f4 * 4, 0.f);
    for (uint32_t b = 0; b < d->n_bsdfs; ++b) bsdfs[((size_t) mask_base + 3u * b + 1u) * 4 + 1] = 1.f;      // no mask: the constant 1
    for (uint32_t k = 0; k < n_masks; ++k) {
        const msk_mask_desc &m = masks[k];
        float *o = &bsdfs[((size_t) mask_base + 3u * m.bsdf) * 4];
        const uint32_t filter = (uint32_t) m.filter;
        std::memcpy(&o[4], &filter, 4);
        if (m.filter == 0) { o[5] = m.opacity; continue; }
        // word 0: the first value's place among the images' values; place_mask_values adds where those start in the pool
        const uint32_t w[3] = {(uint32_t) mask_values.size(), m.width, m.height};
        std::memcpy(&o[0], w, 12); o[3] = m.to_uv[2];
        o[5] = 0.f; o[6] = 0.f; o[7] = m.to_uv[5];
        o[8] = m.to_uv[0]; o[9] = m.to_uv[1]; o[10] = m.to_uv[3]; o[11] = m.to_uv[4];
        mask_values.insert(mask_values.end(), m.values, m.values + (size_t) m.width * m.height);
        has_mask_image = true;
    }
    return MSK_OK;
}

// the images' values behind everything the texel pool holds so far, one float each, padded to a float4; the image records' first word
// becomes an index into the pool read as floats
inline void place_mask_values(uint32_t n_bsdfs, uint32_t mask_base, std::vector<float> &bsdfs, const std::vector<float> &mask_values, std::vector<float> &pool) {
    const uint32_t first = (uint32_t) pool.size();
    for (uint32_t b = 0; b < n_bsdfs; ++b) {
        float *o = &bsdfs[((size_t) mask_base + 3u * b) * 4];
        uint32_t filter, w0;
        std::memcpy(&filter, &o[4], 4);
        if (filter == 0u) continue;
        std::memcpy(&w0, &o[0], 4); w0 += first; std::memcpy(&o[0], &w0, 4);
    }
    pool.insert(pool.end(), mask_values.begin(), mask_values.end());
    pool.resize((pool.size() + 3) & ~(size_t) 3, 0.f);
}

}  // namespace mskscene
