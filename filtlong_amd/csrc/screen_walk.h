// screen_walk.h — what the walks of the contaminant screen's kernels share (device code only; screen.h and screen_hash.h stay host
// headers): the 2-bit codes and validity bits of the bytes of an aligned 16-byte load, and the span -> sequence lookup in the segment
// table.  k_screen_hits (screen.hip) has its own two-load span loop; k_screen_hits_hash and k_screenset_insert share the three-load
// walk_spans of screen_hash.hip.  The bitmap kernel on one templated walk with the hashed ones measured 2 % slower in its "lds" form
// against a small set, so the loops stay apart.
#pragma once

#include "screen_hash.h"

namespace screen_walk {

using screen::kScreenSpan;
using screen::kScreenStep;

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));  // (the compiler's own vector: sixteen bytes that stay in registers)

// the codes of the four bases in a dword of the plane, first base on top (bits 7..0 of the result)
__device__ __forceinline__ uint32_t codes4(uint32_t w) {
    const uint32_t c2 = ((w >> 1) ^ (w >> 2)) & 0x03030303u;  // the code of byte b in bits 8 b + 1 .. 8 b
    return (c2 * 0x40100401u) >> 24;                          // b0 << 30 | b1 << 28 | b2 << 26 | b3 << 24: no two terms overlap
}
__device__ __forceinline__ uint32_t codes16(u32x4 v) { return (codes4(v.x) << 24) | (codes4(v.y) << 16) | (codes4(v.z) << 8) | codes4(v.w); }
__device__ __forceinline__ uint32_t valid4(uint32_t w) {
    uint32_t m = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) m |= (screen::is_acgt((uint8_t)(w >> (8 * b))) ? 1u : 0u) << b;
    return m;
}
__device__ __forceinline__ uint32_t valid16(u32x4 v) { return valid4(v.x) | (valid4(v.y) << 4) | (valid4(v.z) << 8) | (valid4(v.w) << 12); }

// the sequence of span sp in processing order: the largest r with seg_start[r] <= sp (sequences without spans share their
// successor's start and lose)
__device__ __forceinline__ uint32_t span_of(const uint32_t *seg_start, uint32_t n_reads, uint32_t sp) {
    uint32_t lo = 0, hi = n_reads;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (seg_start[mid] <= sp) lo = mid;
        else hi = mid;
    }
    return lo;
}

}  // namespace screen_walk
