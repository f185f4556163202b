// plastic_constants_probe.cpp — the two constants the packer computes for a `plastic` / `roughplastic` entry, on a CPU, for
// tests/test_plastic_oracle_parity.py: mskscene::plastic_constants (csrc/msk_plastic_tables.h) as pack_bsdfs calls it, on the
// msk_scene_desc a test hands to the library.  Built as a shared library and called through ctypes.  The descriptor must be one the
// packer accepts (the tests pass flattened scenes): the function reads the textures, texels and tabulated spectra the entry names.
#include "../../misaki-render_amd/csrc/msk_plastic_tables.h"

// out2 = {fdr_int, ssw}; -1 for an entry out of range or one that is no plastic of either type
extern "C" int plastic_constants_probe(const msk_scene_desc *d, uint32_t bsdf, float *out2) {
    if (bsdf >= d->n_bsdfs) return -1;
    const msk_bsdf_desc &bd = d->bsdfs[bsdf];
    if (bd.type != MSK_BSDF_PLASTIC && bd.type != MSK_BSDF_ROUGHPLASTIC) return -1;
    mskscene::plastic_constants(d, bd, out2);
    return 0;
}
