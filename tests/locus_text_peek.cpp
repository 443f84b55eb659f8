// locus_text_peek.cpp — test helper (tests/test_gpu_locus_text.py): what a finalized k-mer set keeps for the locus path of the cover
// kernels (csrc/kmerset.h: flx_locus), copied to the host.  Built at test time into a shared object and called through ctypes.
#include "kmerset.h"

// info[0] = 1 when the set has a text, then n_alloc, n_text, seed slots, seed_shift, 1 when it has safe1.  With `text` set the
// arrays are copied as well: text (n_alloc x 2 words), safe1 (n_alloc x uint16, when there is one), seed (slots words).
extern "C" int locus_text_peek(const flx_kmerset *set, uint64_t *info, uint32_t *text, uint16_t *safe1, uint32_t *seed) {
    const flx_locus *loc = flx_kmerset_locus(set);
    for (int i = 0; i < 6; ++i) info[i] = 0;
    if (!loc) return 0;
    const uint64_t slots = (uint64_t)loc->seed_mask + 1;
    info[0] = 1;
    info[1] = loc->n_alloc;
    info[2] = loc->n_text;
    info[3] = slots;
    info[4] = (uint64_t)loc->seed_shift;
    info[5] = loc->safe1 ? 1 : 0;
    if (!text) return 0;
    if (hipMemcpy(text, loc->text, (size_t)loc->n_alloc * 8, hipMemcpyDeviceToHost) != hipSuccess) return 1;
    if (loc->safe1 && hipMemcpy(safe1, loc->safe1, (size_t)loc->n_alloc * 2, hipMemcpyDeviceToHost) != hipSuccess) return 2;
    if (hipMemcpy(seed, loc->seed, slots * 4, hipMemcpyDeviceToHost) != hipSuccess) return 3;
    return 0;
}
