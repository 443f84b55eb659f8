// screen.hip — --exclude: how many 16-mers of every read are members of a contaminant set (screen.h has the definition).
//
// The cover kernels of k-mer mode answer which BASES are covered, for reads that come from the reference.  A screen sees the opposite
// population — nearly every read is unrelated to X — and wants one integer per read.  So the work item is not a read but a SPAN of
// kScreenSpan window start positions of one read: a 4 Mbp read is a thousand spans that spread over the whole chip (one
// wave per read took 12.6 ms for such a read), and the hits of a span are added into hits[read] with one integer atomicAdd per wave.
//
//   k_screen_segments   spans per read in processing order, ceil(windows / kScreenSpan); the exclusive scan of sort.hip turns them
//                       into the segment table seg_start[0 .. n_reads], all on the device: no host round trip in front of the kernel
//   k_screen_hits       persistent workgroups of 16 waves; wave w of the grid takes the spans w, w + waves, ...; the read of a span
//                       is found by a binary search in seg_start (wave-uniform; screen_walk.h: span_of).  A span goes 1024 positions
//                       a step: every lane owns 16 consecutive window starts, i.e. the 16 bytes of one aligned 16-byte load plus the
//                       next 15 (a second aligned load, skipped where it would leave [offset, offset + round_up(L, 16))).  The next
//                       step's bytes are requested before this step's are used.  Per lane: the 2-bit codes of its 31 bases in one
//                       64-bit word, a validity bit per byte (screen_walk.h has both, for the hashed kernels too), and from those the
//                       16 windows that consist of ACGTacgt only.
//
// The host side of both kinds of set is here as well (screen_internal.h): screen_hits_dev — the checks, the segment table, the launch
// of k_screen_hits or of screen_hash.hip's kernel — and screen_hits_host, the staged host-array form; flx_screen_hits*,
// flx_screenset_hits* and the pipeline call them with a flx_screen_ref.
//
// Three filters stand in front of the exact answer; none has false negatives, and only the exact bitmap decides a hit:
//   TIER 2 "lds"    the presence bitmap of the 10-mers inside members of X (4^10 bits = 128 KiB), loaded into LDS once per workgroup
//                   (one workgroup per CU).  A window can only be a member if its seven 10-mers are present: the lane looks up the
//                   22 10-mers that start at its bases 0..21 and a window survives on seven consecutive set bits.  The few windows
//                   that leave the LDS ask the 12-mer prefilter (five L2 lookups, ending at the first clear bit), then the bitmap.
//   TIER 1 "pre12"  no LDS table (too full to pay: kmerset.hip has the threshold): the L2-resident 12-mer prefilter, rolled the
//                   same way — 20 lookups per lane, five consecutive set bits — then the bitmap.
//   TIER 0 "exact"  the set has no prefilters (FLX_KMER_PREFILTER=0, or a set too large for them): every valid window asks the bitmap.
#include "rank_internal.h"
#include "screen_internal.h"
#include "screen_walk.h"

namespace {

using screen::kScreenSpan;
using screen::kScreenStep;
using screen_walk::codes4;
using screen_walk::span_of;
using screen_walk::u32x4;
using screen_walk::valid4;

constexpr int kScreenThreads = 1024;  // 16 waves: with the 128 KiB table one workgroup per CU
constexpr int kPre10Words = 1 << 15;  // 4^10 bits

__global__ void __launch_bounds__(256) k_screen_segments(const int32_t *lengths, const uint32_t *order, uint64_t n_reads, int k, uint32_t span,
                                                         uint32_t *counts) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r > n_reads) return;
    uint32_t c = 0;
    if (r < n_reads) {
        const uint32_t read = order ? order[r] : (uint32_t)r;
        c = (screenk::windows_of(lengths[read], k) + span - 1u) / span;
    }
    counts[r] = c;  // counts[n_reads] = 0: its scanned value is the number of spans
}

__device__ __forceinline__ uint32_t bit_of(const uint32_t *bm, uint32_t k) { return (bm[k >> 5] >> (k & 31)) & 1u; }

template <int TIER>
__global__ void __launch_bounds__(kScreenThreads) k_screen_hits(const uint8_t *__restrict__ plane, const uint64_t *__restrict__ offsets,
                                                                const int32_t *__restrict__ lengths, const uint32_t *__restrict__ order,
                                                                uint32_t n_reads, const uint32_t *__restrict__ seg_start,
                                                                const uint32_t *__restrict__ bitmap, const uint32_t *__restrict__ pre12,
                                                                const uint32_t *__restrict__ pre10, uint32_t *hits) {
    __shared__ uint32_t s_tab[TIER == 2 ? kPre10Words : 1];
    if (TIER == 2) {
        const u32x4 *src = (const u32x4 *)pre10;
        u32x4 *dst = (u32x4 *)s_tab;
        for (int i = threadIdx.x; i < kPre10Words / 4; i += kScreenThreads) dst[i] = src[i];
        __syncthreads();
    }
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t n_waves = gridDim.x * (kScreenThreads / 64);
    const uint32_t total = seg_start[n_reads];
    const u32x4 zero = {0u, 0u, 0u, 0u};  // (a zero byte is not in ACGTacgt)

    for (uint32_t sp = blockIdx.x * (kScreenThreads / 64) + wave; sp < total; sp += n_waves) {
        const uint32_t lo = span_of(seg_start, n_reads, sp);
        const uint32_t read = order ? order[lo] : lo;
        const uint32_t len = (uint32_t)lengths[read];     // at least 16: the read has a span
        const uint32_t lpad = (len + 15u) & ~15u;         // loads stay inside [offset, offset + lpad)
        const uint32_t w0 = (sp - seg_start[lo]) * (uint32_t)kScreenSpan;
        const uint32_t w1 = min(len - 15u, w0 + (uint32_t)kScreenSpan);  // this span: window starts [w0, w1)
        const uint8_t *base = plane + offsets[read];

        uint32_t p = w0 + lane * 16u;  // a multiple of 16; p < w1 <= len - 15 puts the first load inside the read
        u32x4 a = p < w1 ? *(const u32x4 *)(base + p) : zero;
        u32x4 b = (p < w1 && p + 16u < lpad) ? *(const u32x4 *)(base + p + 16u) : zero;
        uint32_t count = 0;
        for (uint32_t sb = w0; sb < w1; sb += (uint32_t)kScreenStep, p += (uint32_t)kScreenStep) {
            const uint32_t pn = p + (uint32_t)kScreenStep;  // the next step's bytes, requested before this step's are used
            const u32x4 na = pn < w1 ? *(const u32x4 *)(base + pn) : zero;
            const u32x4 nb = (pn < w1 && pn + 16u < lpad) ? *(const u32x4 *)(base + pn + 16u) : zero;
            if (p < w1) {
                // bases 0..30 of the lane: base k in bits 2 (30 - k) + 1 .. 2 (30 - k) of `codes`, bit k of `vm` = byte k is in ACGTacgt
                const uint32_t hi16 = (codes4(a.x) << 24) | (codes4(a.y) << 16) | (codes4(a.z) << 8) | codes4(a.w);
                const uint32_t lo16 = (codes4(b.x) << 24) | (codes4(b.y) << 16) | (codes4(b.z) << 8) | codes4(b.w);
                const uint64_t codes = ((uint64_t)hi16 << 30) | (uint64_t)(lo16 >> 2);
                const uint32_t vm = (valid4(a.x) | (valid4(a.y) << 4) | (valid4(a.z) << 8) | (valid4(a.w) << 12) | (valid4(b.x) << 16) |
                                     (valid4(b.y) << 20) | (valid4(b.z) << 24) | (valid4(b.w) << 28)) & 0x7FFFFFFFu;
                // bit j: the 16 bytes from base j on are all valid, and the window start p + j lies in the span
                uint32_t wv = vm & (vm >> 1);
                wv &= wv >> 2;
                wv &= wv >> 4;
                wv &= wv >> 8;
                wv &= 0xFFFFu;
                const uint32_t left = w1 - p;
                if (left < 16u) wv &= (1u << left) - 1u;
                if (TIER == 2 && wv) {
                    uint32_t m = 0;
#pragma unroll
                    for (int k = 0; k < 22; ++k) {  // the 10-mer from base k on
                        const uint32_t t = (uint32_t)(codes >> (2 * (21 - k))) & 0xFFFFFu;
                        m |= bit_of(s_tab, t) << k;
                    }
                    m &= m >> 1;
                    m &= m >> 2;
                    m &= m >> 3;  // bit j: the seven 10-mers from bases j .. j + 6 on are present
                    wv &= m;
                }
                if (TIER == 1 && wv) {
                    uint32_t m = 0;
#pragma unroll
                    for (int k = 0; k < 20; ++k) {  // the 12-mer from base k on
                        const uint32_t t = (uint32_t)(codes >> (2 * (19 - k))) & 0xFFFFFFu;
                        m |= bit_of(pre12, t) << k;
                    }
                    uint32_t m4 = m & (m >> 1);
                    m4 &= m4 >> 2;
                    wv &= m4 & (m >> 4);  // bit j: the five 12-mers from bases j .. j + 4 on are present
                }
                if (TIER == 0) {
#pragma unroll
                    for (int j = 0; j < 16; ++j) {  // (sixteen independent lookups; a window that is not valid asks word 0 and is masked)
                        const uint32_t on = (wv >> j) & 1u;
                        const uint32_t k = on ? (uint32_t)(codes >> (2 * (15 - j))) : 0u;
                        count += bit_of(bitmap, k) & on;
                    }
                } else {
                    while (wv) {
                        const int j = __ffs(wv) - 1;
                        wv &= wv - 1u;
                        const uint32_t k = (uint32_t)(codes >> (2 * (15 - j)));
                        bool maybe = true;
                        if (TIER == 2 && pre12) {
                            for (int d = 0; d < 5 && maybe; ++d) maybe = bit_of(pre12, flx_sub12(k, d)) != 0u;
                        }
                        if (maybe) count += bit_of(bitmap, k);
                    }
                }
            }
            a = na;
            b = nb;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) count += __shfl_xor(count, o, 64);
        if (lane == 0 && count) atomicAdd(&hits[read], count);
    }
}

__global__ void __launch_bounds__(256) k_screen_apply(uint64_t n_reads, const int32_t *lengths, const uint32_t *hits, uint64_t t, int k,
                                                      uint8_t *passed, const uint64_t *child_offsets, uint8_t *child_passed, uint8_t *excluded) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_reads) return;
    const bool out = screen::excluded(hits[i], screenk::windows_of(lengths[i], k), t);
    excluded[i] = out ? 1 : 0;
    if (!out) return;
    passed[i] = 0;
    if (child_offsets)
        for (uint64_t c = child_offsets[i]; c < child_offsets[i + 1]; ++c) child_passed[c] = 0;
}

}  // namespace

// the spans of every read in processing order for windows of k bases, counts[0 .. n] (the last is 0), and their exclusive scan: no
// host round trip in front of a walk (screen_hits_dev below, flx_screenset_add; complexity.hip with spans of its own)
int flx_screen_segment_table(flx_ctx *ctx, const int32_t *d_lengths, const uint32_t *d_order, uint64_t n, int k, uint32_t **seg_start, uint32_t span) {
    const size_t table = ((n + 1) * 4 + 255) & ~(size_t)255;
    const size_t scan_ws = ((n + 1) / 2048 + 4096) * 8;
    void *scr;
    FLX_CHECK(flx_scratch(ctx, 2 * table + scan_ws, &scr));
    uint32_t *counts = (uint32_t *)scr;
    *seg_start = (uint32_t *)((char *)scr + table);
    hipLaunchKernelGGL(k_screen_segments, dim3((unsigned)((n + 1 + 255) / 256)), dim3(256), 0, ctx->stream, d_lengths, d_order, n, k, span, counts);
    FLX_HIP(ctx, hipGetLastError());
    return flx_exclusive_scan_u32(ctx, n + 1, counts, *seg_start, (char *)scr + 2 * table, scan_ws);
}

// An excluded read is a read that fails a hard cut-off: its pass flag and those of its children are cleared on the device, on the
// context's stream, before anything is copied back (pipeline.hip).
int flx_screen_apply_dev(flx_ctx *ctx, uint64_t n_reads, const int32_t *d_lengths, const uint32_t *d_hits, uint64_t t, int k,
                         uint8_t *d_passed, const uint64_t *d_child_offsets, uint8_t *d_child_passed, uint8_t *d_excluded) {
    if (n_reads == 0) return FLX_OK;
    flx_time_begin(ctx, "flx_screen_apply");
    hipLaunchKernelGGL(k_screen_apply, dim3((unsigned)((n_reads + 255) / 256)), dim3(256), 0, ctx->stream, n_reads, d_lengths, d_hits, t, k,
                       d_passed, d_child_offsets, d_child_passed, d_excluded);
    flx_time_end(ctx);
    FLX_HIP(ctx, hipGetLastError());
    return FLX_OK;
}

extern "C" int flx_screen_threshold(double percent, uint64_t *t) {
    if (!t || !screen::threshold(percent, t)) return FLX_ERR_INVALID;
    return FLX_OK;
}

extern "C" uint32_t flx_screen_span(void) { return (uint32_t)kScreenSpan; }

extern "C" const char *flx_last_screen_filter(const flx_ctx *ctx) { return ctx ? ctx->last_screen_filter : ""; }

extern "C" int flx_screen_set_add(flx_kmerset *set, const uint8_t *bases, const uint64_t *offsets, const int64_t *lengths, uint64_t n_seqs) {
    if (!set) return FLX_ERR_INVALID;
    flx_ctx *ctx = flx_kmerset_ctx(set);
    if (n_seqs && (!bases || !offsets || !lengths)) return flx_fail(ctx, FLX_ERR_INVALID, "NULL sequence arrays");
    for (uint64_t i = 0; i < n_seqs; ++i)
        if (lengths[i] < 0) return flx_fail(ctx, FLX_ERR_INVALID, "negative sequence length");
    std::vector<uint64_t> piece_offsets;
    std::vector<int64_t> piece_lengths;
    screen::split_acgt(bases, offsets, lengths, n_seqs, &piece_offsets, &piece_lengths);
    flx_kmerset_mark_screen(set);  // finalize then builds the 10-mer table as well
    if (piece_offsets.empty()) return FLX_OK;
    return flx_kmerset_add_assembly(set, bases, piece_offsets.data(), piece_lengths.data(), piece_offsets.size());
}

namespace {

int check_set(flx_ctx *ctx, flx_screen_ref ref) {
    if (!ref.is_final()) return flx_fail(ctx, FLX_ERR_STATE, "the set to screen against is not finalized");
    if (ref.size() == 0) return flx_fail(ctx, FLX_ERR_STATE, "the set to screen against is empty (no run of %d bases of ACGT in it)", ref.k());
    return FLX_OK;
}

// k_screen_hits<tier> for the filters the set has, over a finished segment table
int launch_bitmap_hits(flx_ctx *ctx, const flx_kmerset *set, const void *d_plane, const void *d_offsets, const void *d_lengths, const void *d_order,
                       uint64_t n_reads, const uint32_t *seg_start, uint32_t *d_hits) {
    const uint32_t *pre10 = flx_kmerset_pre10(set), *pre12 = flx_kmerset_prefilter(set);
    const int tier = pre10 ? 2 : pre12 ? 1 : 0;
    ctx->last_screen_filter = tier == 2 ? "lds" : tier == 1 ? "pre12" : "exact";
    const unsigned n_cu = (unsigned)ctx->prop.multiProcessorCount;
#define FLX_SCREEN_LAUNCH(T, blocks)                                                                                                                \
    hipLaunchKernelGGL(k_screen_hits<T>, dim3(blocks), dim3(kScreenThreads), 0, ctx->stream, (const uint8_t *)d_plane, (const uint64_t *)d_offsets, \
                       (const int32_t *)d_lengths, (const uint32_t *)d_order, (uint32_t)n_reads, seg_start, flx_kmerset_bitmap(set), pre12, pre10, d_hits)
    if (tier == 2) FLX_SCREEN_LAUNCH(2, n_cu);  // the table fills the LDS of a CU: one workgroup each
    else if (tier == 1) FLX_SCREEN_LAUNCH(1, 2 * n_cu);
    else FLX_SCREEN_LAUNCH(0, 2 * n_cu);
#undef FLX_SCREEN_LAUNCH
    FLX_HIP(ctx, hipGetLastError());
    return FLX_OK;
}

}  // namespace

int screen_hits_dev(flx_ctx *ctx, flx_screen_ref ref, const void *d_plane, uint64_t plane_bytes, const void *d_offsets, const void *d_lengths,
                    const void *d_order, uint64_t n_reads, uint32_t *d_hits) {
    FLX_CHECK(check_set(ctx, ref));
    if (n_reads > 0xfffffffeull) return flx_fail(ctx, FLX_ERR_INVALID, "at most 2^32-2 reads per batch");
    if (plane_bytes & 15) return flx_fail(ctx, FLX_ERR_INVALID, "plane_bytes must be a multiple of 16");
    if (n_reads == 0) return FLX_OK;
    if (!d_plane || !d_offsets || !d_lengths || !d_hits) return flx_fail(ctx, FLX_ERR_INVALID, "plane/offsets/lengths/hits must not be NULL");
    if (plane_bytes / (uint64_t)kScreenSpan + n_reads > 0xffffffffull) return flx_fail(ctx, FLX_ERR_INVALID, "too many spans in one batch");
    FLX_HIP(ctx, hipSetDevice(ctx->device));
    flx_time_scope timed(ctx, "flx_screen");
    FLX_HIP(ctx, hipMemsetAsync(d_hits, 0, n_reads * 4, ctx->stream));
    uint32_t *seg_start = nullptr;
    FLX_CHECK(flx_screen_segment_table(ctx, (const int32_t *)d_lengths, (const uint32_t *)d_order, n_reads, ref.k(), &seg_start));
    if (ref.hashed) FLX_CHECK(flx_screenset_launch_hits(ctx, ref.hashed, d_plane, d_offsets, d_lengths, d_order, n_reads, seg_start, d_hits));
    else FLX_CHECK(launch_bitmap_hits(ctx, ref.bitmap, d_plane, d_offsets, d_lengths, d_order, n_reads, seg_start, d_hits));
    timed.end();
    return FLX_OK;
}

// the host-array form: everything staged through device buffers of the call's own
int screen_hits_host(flx_ctx *ctx, flx_screen_ref ref, const uint8_t *plane, uint64_t plane_bytes, const uint64_t *offsets, const int32_t *lengths,
                     const uint32_t *order, uint64_t n_reads, uint32_t *hits) {
    FLX_CHECK(check_set(ctx, ref));
    if (plane_bytes & 15) return flx_fail(ctx, FLX_ERR_INVALID, "plane_bytes must be a multiple of 16");
    if (n_reads == 0) return FLX_OK;
    if (!plane || !offsets || !lengths || !hits) return flx_fail(ctx, FLX_ERR_INVALID, "plane/offsets/lengths/hits must not be NULL");
    FLX_CHECK(flx_check_reads(ctx, plane_bytes, offsets, lengths, order, n_reads));  // (the kernel adds every span of every read exactly once)
    FLX_HIP(ctx, hipSetDevice(ctx->device));
    flx_dbuf d_plane, d_off, d_len, d_ord, d_hits;
    FLX_CHECK(flx_dalloc(ctx, d_plane, plane_bytes ? plane_bytes : 16));
    FLX_CHECK(flx_dalloc(ctx, d_off, n_reads * 8));
    FLX_CHECK(flx_dalloc(ctx, d_len, n_reads * 4));
    FLX_CHECK(flx_dalloc(ctx, d_hits, n_reads * 4));
    if (plane_bytes) FLX_HIP(ctx, hipMemcpyAsync(d_plane.p, plane, plane_bytes, hipMemcpyHostToDevice, ctx->stream));
    FLX_HIP(ctx, hipMemcpyAsync(d_off.p, offsets, n_reads * 8, hipMemcpyHostToDevice, ctx->stream));
    FLX_HIP(ctx, hipMemcpyAsync(d_len.p, lengths, n_reads * 4, hipMemcpyHostToDevice, ctx->stream));
    if (order) {
        FLX_CHECK(flx_dalloc(ctx, d_ord, n_reads * 4));
        FLX_HIP(ctx, hipMemcpyAsync(d_ord.p, order, n_reads * 4, hipMemcpyHostToDevice, ctx->stream));
    }
    // (a pattern no count can be: a kernel that wrote nothing must not hand back an earlier call's answers — score_api.hip)
    FLX_HIP(ctx, hipMemsetAsync(d_hits.p, 0xA5, n_reads * 4, ctx->stream));
    FLX_CHECK(screen_hits_dev(ctx, ref, d_plane.p, plane_bytes, d_off.p, d_len.p, order ? d_ord.p : nullptr, n_reads, d_hits.as<uint32_t>()));
    FLX_HIP(ctx, hipMemcpyAsync(hits, d_hits.p, n_reads * 4, hipMemcpyDeviceToHost, ctx->stream));
    FLX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return FLX_OK;
}

extern "C" int flx_screen_hits_dev(flx_ctx *ctx, const flx_kmerset *set, const void *d_plane, uint64_t plane_bytes, const void *d_offsets,
                                   const void *d_lengths, const void *d_order, uint64_t n_reads, uint32_t *d_hits) {
    if (!ctx) return FLX_ERR_INVALID;
    if (!set) return flx_fail(ctx, FLX_ERR_INVALID, "flx_screen_hits: set must not be NULL");
    return screen_hits_dev(ctx, flx_screen_ref{set, nullptr}, d_plane, plane_bytes, d_offsets, d_lengths, d_order, n_reads, d_hits);
}

extern "C" int flx_screen_hits(flx_ctx *ctx, const flx_kmerset *set, const uint8_t *plane, uint64_t plane_bytes, const uint64_t *offsets,
                               const int32_t *lengths, const uint32_t *order, uint64_t n_reads, uint32_t *hits) {
    if (!ctx) return FLX_ERR_INVALID;
    if (!set) return flx_fail(ctx, FLX_ERR_INVALID, "flx_screen_hits: set must not be NULL");
    return screen_hits_host(ctx, flx_screen_ref{set, nullptr}, plane, plane_bytes, offsets, lengths, order, n_reads, hits);
}
