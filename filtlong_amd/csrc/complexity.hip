// complexity.hip — --max_low_complexity: how many 64-base windows of every read are bad, i.e. score above the threshold on the
// triplet-pair score of DUST at one fixed window length (complexity.h has the definition).
//
// The work item is, as for the screen, a SPAN of one read — kSpan window start positions — found through the segment table of
// screen.hip (flx_screen_segment_table with k = 64 and this file's span), so one very long read spreads over the whole chip and the
// bad windows of a span are added into bad[read] with one integer atomicAdd per wave.
//
//   k_complexity_bad    persistent workgroups of 4 waves; wave w of the grid takes the spans w, w + waves, ...  Inside a span every
//                       lane owns kLaneRun = 128 consecutive window starts [s0, s1) — in the last span of a read a 64th of what is
//                       left, in whole 16s (complexity.h: lane_run) — begins with an empty state at base s0 and walks the bases
//                       s0 .. s1 + 62 (complexity.h: the piece-wise walk, which is exact because the state of a window is a
//                       function of its 64 bytes alone).  The first 63 bases are the warm-up: a third of a whole run's walk.
//                       Bytes: one aligned 16-byte load per 16 bases and lane, the next one requested before this one is used; a
//                       load is only issued where the lane still needs a byte of it, which keeps it inside [offset, offset +
//                       round_up(L, 16)).  History: the 2-bit codes of the last 80 bases in five dwords and their validity bits in
//                       five more, rotated once per 16 bases, so the triplet that leaves (64 bases back) and the one that enters are
//                       static shifts of two 64-bit words.  Counters: 64 per lane, one byte each (at most 62), in LDS as
//                       s_cnt[wave][t >> 2][lane] — the dword of lane l is in bank l, so the byte reads and writes of a wave never
//                       conflict whatever the triplets are.  Per base: two LDS byte reads, two byte writes, and about twenty
//                       integer instructions; no floating point.
//   k_complexity_apply  a flagged read is a read that fails a hard cut-off: passed and child_passed cleared, the flag written.
#include "complexity_internal.h"
#include "screen_internal.h"
#include "screen_walk.h"

namespace {

using complexity::kLaneRun;
using complexity::kSpan;
using complexity::kWarmup;
using screen_walk::codes16;
using screen_walk::span_of;
using screen_walk::u32x4;
using screen_walk::valid16;

constexpr int kComplexityThreads = 256;  // 4 waves, 16 KiB of counters
constexpr int kComplexityWaves = kComplexityThreads / 64;
constexpr int kComplexityBlocksPerCU = 8;
constexpr int kLaneLoads = (kLaneRun + kWarmup + 15) / 16;  // 16-byte loads of a lane with a whole run

// byte offset of counter t inside a lane's column of s_cnt (16 rows of 64 dwords)
__device__ __forceinline__ uint32_t slot_of(uint32_t t) { return ((t & 60u) << 6) | (t & 3u); }

__global__ void __launch_bounds__(kComplexityThreads) k_complexity_bad(const uint8_t *__restrict__ plane, const uint64_t *__restrict__ offsets,
                                                                       const int32_t *__restrict__ lengths, const uint32_t *__restrict__ order,
                                                                       uint32_t n_reads, const uint32_t *__restrict__ seg_start, uint32_t t61,
                                                                       uint32_t *bad) {
    __shared__ uint32_t s_cnt[kComplexityWaves][16][64];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t n_waves = gridDim.x * kComplexityWaves;
    const uint32_t total = seg_start[n_reads];
    const u32x4 zero = {0u, 0u, 0u, 0u};
    uint8_t *cnt = (uint8_t *)&s_cnt[wave][0][lane];

    for (uint32_t sp = blockIdx.x * kComplexityWaves + wave; sp < total; sp += n_waves) {
        const uint32_t lo = span_of(seg_start, n_reads, sp);
        const uint32_t read = order ? order[lo] : lo;
        const uint32_t len = (uint32_t)lengths[read];  // at least 64: the read has a span
        const uint32_t w0 = (sp - seg_start[lo]) * (uint32_t)kSpan;
        const uint32_t w1 = min(len - (uint32_t)kWarmup, w0 + (uint32_t)kSpan);  // this span: window starts [w0, w1)
        const uint32_t run = complexity::lane_run(w1 - w0);                     // kLaneRun but in a read's last span
        const uint32_t s0 = w0 + lane * run;                                     // this lane: window starts [s0, s1)
        const uint32_t s1 = min(w1, s0 + run);
        const uint32_t qe = s0 < w1 ? s1 - s0 + (uint32_t)kWarmup : 0u;  // the lane walks the bases s0 + [0, qe); s0 + qe <= len
        const uint32_t nj = (min(w1 - w0, run) + (uint32_t)kWarmup + 15u) >> 4;  // (wave-uniform: lane 0's loads)
        const uint8_t *base = plane + offsets[read] + s0;  // a multiple of 16 past a 16-byte aligned offset

#pragma unroll
        for (int g = 0; g < 16; ++g) s_cnt[wave][g][lane] = 0u;
        u32x4 nxt = qe ? *(const u32x4 *)base : zero;
        uint32_t cw0 = 0, cw1 = 0, cw2 = 0, cw3 = 0, cw4 = 0;  // codes of 16 bases each, first base on top; cw4 is the newest
        uint32_t iv0 = 0, iv1 = 0, iv2 = 0, iv3 = 0, iv4 = 0;  // bit b: byte b of those 16 is outside ACGTacgt
        uint32_t S = 0, invalid = 0, count = 0;
        for (uint32_t j = 0; j < nj; ++j) {
            const u32x4 cur = nxt;
            const uint32_t qn = (j + 1u) << 4;  // the next 16 bytes, requested before these are used
            nxt = qn < qe ? *(const u32x4 *)(base + qn) : zero;
            cw0 = cw1; cw1 = cw2; cw2 = cw3; cw3 = cw4; cw4 = codes16(cur);
            iv0 = iv1; iv1 = iv2; iv2 = iv3; iv3 = iv4; iv4 = ~valid16(cur) & 0xFFFFu;
            const uint64_t x = ((uint64_t)cw0 << 32) | cw1;  // base q - 64 is base b of x
            const uint64_t y = ((uint64_t)cw3 << 32) | cw4;  // base q is base 16 + b of y
            const bool sliding = j >= 4u;                    // q >= 64: a byte and a triplet leave
#pragma unroll
            for (int b = 0; b < 16; ++b) {
                if (sliding) {
                    const uint32_t a = slot_of((uint32_t)(x >> (58 - 2 * b)) & 63u);  // the triplet that began 64 bases back
                    const uint32_t c = (uint32_t)cnt[a] - 1u;
                    cnt[a] = (uint8_t)c;
                    S -= c;
                    invalid -= (iv0 >> b) & 1u;
                }
                invalid += (iv4 >> b) & 1u;
                if (j > 0u || b >= 2) {
                    const uint32_t a = slot_of((uint32_t)(y >> (30 - 2 * b)) & 63u);  // the triplet that ends here
                    const uint32_t c = cnt[a];
                    cnt[a] = (uint8_t)(c + 1u);
                    S += c;
                }
                const uint32_t q = (j << 4) + (uint32_t)b;  // the window that ends here starts at s0 + q - 63
                if (q >= (uint32_t)kWarmup && q < qe && invalid == 0u && 10u * S > t61) ++count;
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) count += __shfl_xor(count, o, 64);
        if (lane == 0 && count) atomicAdd(&bad[read], count);
    }
}

__global__ void __launch_bounds__(256) k_complexity_apply(uint64_t n_reads, const int32_t *lengths, const uint32_t *bad, uint64_t t, uint8_t *passed,
                                                          const uint64_t *child_offsets, uint8_t *child_passed, uint8_t *flagged) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_reads) return;
    const bool out = complexity::flagged(bad[i], complexity::windows_of(lengths[i]), t);
    flagged[i] = out ? 1 : 0;
    if (!out) return;
    passed[i] = 0;
    if (child_offsets)
        for (uint64_t c = child_offsets[i]; c < child_offsets[i + 1]; ++c) child_passed[c] = 0;
}

static_assert(kLaneLoads * 16 >= kLaneRun + kWarmup, "a lane's loads cover its walk");

}  // namespace

int flx_complexity_apply_dev(flx_ctx *ctx, uint64_t n_reads, const int32_t *d_lengths, const uint32_t *d_bad, uint64_t t, uint8_t *d_passed,
                             const uint64_t *d_child_offsets, uint8_t *d_child_passed, uint8_t *d_flagged) {
    if (n_reads == 0) return FLX_OK;
    flx_time_begin(ctx, "flx_complexity_apply");
    hipLaunchKernelGGL(k_complexity_apply, dim3((unsigned)((n_reads + 255) / 256)), dim3(256), 0, ctx->stream, n_reads, d_lengths, d_bad, t,
                       d_passed, d_child_offsets, d_child_passed, d_flagged);
    flx_time_end(ctx);
    FLX_HIP(ctx, hipGetLastError());
    return FLX_OK;
}

extern "C" uint32_t flx_complexity_window(void) { return (uint32_t)complexity::kWindow; }

extern "C" uint32_t flx_complexity_span(void) { return (uint32_t)kSpan; }

extern "C" int flx_complexity_bad_dev(flx_ctx *ctx, const void *d_plane, uint64_t plane_bytes, const void *d_offsets, const void *d_lengths,
                                      const void *d_order, uint64_t n_reads, int score_t, uint32_t *d_bad) {
    if (!ctx) return FLX_ERR_INVALID;
    if (!complexity::score_valid(score_t)) return flx_fail(ctx, FLX_ERR_INVALID, "low_complexity_score must be an integer between 10 and 300");
    if (n_reads > 0xfffffffeull) return flx_fail(ctx, FLX_ERR_INVALID, "at most 2^32-2 reads per batch");
    if (plane_bytes & 15) return flx_fail(ctx, FLX_ERR_INVALID, "plane_bytes must be a multiple of 16");
    if (n_reads == 0) return FLX_OK;
    if (!d_plane || !d_offsets || !d_lengths || !d_bad) return flx_fail(ctx, FLX_ERR_INVALID, "plane/offsets/lengths/bad must not be NULL");
    if (plane_bytes / (uint64_t)kSpan + n_reads > 0xffffffffull) return flx_fail(ctx, FLX_ERR_INVALID, "too many spans in one batch");
    FLX_HIP(ctx, hipSetDevice(ctx->device));
    flx_time_scope timed(ctx, "flx_complexity");
    FLX_HIP(ctx, hipMemsetAsync(d_bad, 0, n_reads * 4, ctx->stream));
    uint32_t *seg_start = nullptr;
    FLX_CHECK(flx_screen_segment_table(ctx, (const int32_t *)d_lengths, (const uint32_t *)d_order, n_reads, complexity::kWindow, &seg_start,
                                       (uint32_t)kSpan));
    const unsigned n_cu = (unsigned)ctx->prop.multiProcessorCount;
    hipLaunchKernelGGL(k_complexity_bad, dim3(kComplexityBlocksPerCU * n_cu), dim3(kComplexityThreads), 0, ctx->stream, (const uint8_t *)d_plane,
                       (const uint64_t *)d_offsets, (const int32_t *)d_lengths, (const uint32_t *)d_order, (uint32_t)n_reads, seg_start,
                       (uint32_t)score_t * (uint32_t)(complexity::kWindow - 3), d_bad);
    FLX_HIP(ctx, hipGetLastError());
    timed.end();
    return FLX_OK;
}

// the host-array form: everything staged through device buffers of the call's own
extern "C" int flx_complexity_bad(flx_ctx *ctx, const uint8_t *plane, uint64_t plane_bytes, const uint64_t *offsets, const int32_t *lengths,
                                  const uint32_t *order, uint64_t n_reads, int score_t, uint32_t *bad) {
    if (!ctx) return FLX_ERR_INVALID;
    if (!complexity::score_valid(score_t)) return flx_fail(ctx, FLX_ERR_INVALID, "low_complexity_score must be an integer between 10 and 300");
    if (plane_bytes & 15) return flx_fail(ctx, FLX_ERR_INVALID, "plane_bytes must be a multiple of 16");
    if (n_reads == 0) return FLX_OK;
    if (!plane || !offsets || !lengths || !bad) return flx_fail(ctx, FLX_ERR_INVALID, "plane/offsets/lengths/bad must not be NULL");
    FLX_CHECK(flx_check_reads(ctx, plane_bytes, offsets, lengths, order, n_reads));  // (the kernel adds every span of every read exactly once)
    FLX_HIP(ctx, hipSetDevice(ctx->device));
    flx_dbuf d_plane, d_off, d_len, d_ord, d_bad;
    FLX_CHECK(flx_dalloc(ctx, d_plane, plane_bytes ? plane_bytes : 16));
    FLX_CHECK(flx_dalloc(ctx, d_off, n_reads * 8));
    FLX_CHECK(flx_dalloc(ctx, d_len, n_reads * 4));
    FLX_CHECK(flx_dalloc(ctx, d_bad, n_reads * 4));
    if (plane_bytes) FLX_HIP(ctx, hipMemcpyAsync(d_plane.p, plane, plane_bytes, hipMemcpyHostToDevice, ctx->stream));
    FLX_HIP(ctx, hipMemcpyAsync(d_off.p, offsets, n_reads * 8, hipMemcpyHostToDevice, ctx->stream));
    FLX_HIP(ctx, hipMemcpyAsync(d_len.p, lengths, n_reads * 4, hipMemcpyHostToDevice, ctx->stream));
    if (order) {
        FLX_CHECK(flx_dalloc(ctx, d_ord, n_reads * 4));
        FLX_HIP(ctx, hipMemcpyAsync(d_ord.p, order, n_reads * 4, hipMemcpyHostToDevice, ctx->stream));
    }
    // (a pattern no count can be: a kernel that wrote nothing must not hand back an earlier call's answers — score_api.hip)
    FLX_HIP(ctx, hipMemsetAsync(d_bad.p, 0xA5, n_reads * 4, ctx->stream));
    FLX_CHECK(flx_complexity_bad_dev(ctx, d_plane.p, plane_bytes, d_off.p, d_len.p, order ? d_ord.p : nullptr, n_reads, score_t, d_bad.as<uint32_t>()));
    FLX_HIP(ctx, hipMemcpyAsync(bad, d_bad.p, n_reads * 4, hipMemcpyDeviceToHost, ctx->stream));
    FLX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return FLX_OK;
}
