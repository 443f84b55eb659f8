// endtrim.hip — --trim_ends_q on the GPU: where the low-quality head and tail of every read end (the definition: endtrim.h).
//
// One byte a base is read and an associative integer reduction is taken over it, so the work item is, as for the screen and the
// low-complexity filter, a SPAN of one read — endtrim::kSpan quality bytes — found through the segment table of screen.hip
// (flx_screen_segment_table with windows of one base and this file's span): a batch of 10 kbp reads is one wave per read, one very
// long read spreads over the whole chip.
//
//   k_endtrim_spans   persistent workgroups of 4 waves; wave w of the grid takes the spans w, w + waves, ...  A span goes 1024 bases a
//                     step: lane l takes the 16 bases from p0 + 16 l with one aligned 16-byte load, the next step's bytes requested
//                     before this step's are used.  The lane walks its run (endtrim.h: the piece of a run of bases — the sum, the
//                     best prefix and where it ends, the best suffix and where it begins), E out of the 1 KiB table in LDS; the 64
//                     pieces of a step are combined in order by a shuffle tree (the rule is associative, not commutative: the lane
//                     in front is always the left operand) and lane 0 appends the step's piece to the span's.  A read of one span
//                     is finished here: lane 0 writes its two cuts.  Otherwise the span's piece goes to partials[span].
//   k_endtrim_reads   one wave per read: a read without a base gets 0, 0; a read of several spans has its partials combined in
//                     order — every lane a run of consecutive spans, then the same tree — and lane 0 writes the cuts.  The kernel
//                     boundary in front of it is what makes the partials visible; there is no hand-off inside a launch.
//   bounds            a load reads 16 bytes at offset + p with p a multiple of 16 below L, so inside [offset, offset + round_up(L,
//                     16)); cuts[2 r] and cuts[2 r + 1] are written by the one wave that owns read r; partials[sp] only for sp below
//                     the number the host made room for.
//   children          k_endtrim_children turns the two cuts into the child CSR's count, first and last (endtrim.h: child_of), and
//                     k_endtrim_emit writes the one range.  Everything behind that — the child plane, the children's scoring — is
//                     the code --split_window_q and --trim_adapters run (qsplit.hip: flx_phred_children).
#include "flx_internal.h"
#include "endtrim.h"
#include "rank_internal.h"
#include "screen_internal.h"
#include "screen_walk.h"

namespace {

using endtrim::kSpan;
using endtrim::Piece;
using screen_walk::span_of;
using screen_walk::u32x4;

__constant__ uint32_t c_endtrim_table[256] = {QSPLIT_ERROR_TABLE};

constexpr int kEndtrimThreads = 256;  // 4 waves
constexpr int kEndtrimWaves = kEndtrimThreads / 64;
constexpr int kEndtrimBlocksPerCU = 5;  // what 82 registers a lane leave resident: 5 waves per SIMD
constexpr int kLaneBases = 16;               // bases per lane and step: one 16-byte load
constexpr int kStepBases = 64 * kLaneBases;  // bases per wave and step

static_assert(kSpan % kStepBases == 0, "a span is whole steps, so every load of a span is 16-byte aligned");

struct SpanArgs {
    const uint8_t *plane;
    const uint64_t *offsets;
    const int32_t *lengths;
    const uint32_t *order;
    uint32_t n_reads;
    const uint32_t *seg_start;  // [n_reads + 1], processing order
    uint64_t t;
    Piece *partials;  // [max_partials], by span
    uint32_t max_partials;
    uint32_t *cuts;  // [2 n_reads], input order
};

__device__ __forceinline__ Piece shfl_down_piece(const Piece &p, unsigned o) {
    Piece q;
    q.sum = (int64_t)__shfl_down((unsigned long long)p.sum, o, 64);
    q.pre = (int64_t)__shfl_down((unsigned long long)p.pre, o, 64);
    q.suf = (int64_t)__shfl_down((unsigned long long)p.suf, o, 64);
    q.pre_at = __shfl_down(p.pre_at, o, 64);
    q.suf_at = __shfl_down(p.suf_at, o, 64);
    return q;
}

// the pieces of the 64 lanes, adjacent in lane order, combined into lane 0's
__device__ __forceinline__ Piece wave_combine(Piece p, uint32_t lane) {
#pragma unroll
    for (unsigned o = 1; o < 64; o <<= 1) {
        const Piece q = shfl_down_piece(p, o);
        if ((lane & (2u * o - 1u)) == 0u) p = endtrim::combine(p, q);
    }
    return p;
}

// the piece of the lane's 16 bytes, the bases [pos, min(pos + 16, s1)); GUARD: the run may end inside them
template <bool GUARD>
__device__ __forceinline__ Piece lane_piece(const u32x4 v, const uint32_t *tab, uint32_t pos, uint32_t s1, uint64_t t) {
    Piece p = endtrim::empty_at(GUARD && pos > s1 ? s1 : pos);
    int64_t run = 0, lo = 0;
    uint32_t lo_at = p.pre_at;
    const uint32_t w4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 0; k < kLaneBases; ++k) {
        const uint32_t b = (w4[k >> 2] >> (8 * (k & 3))) & 0xffu;
        const bool in = !GUARD || pos + (uint32_t)k < s1;
        if (in) run += endtrim::weight(tab[b], t);
        if (in && run > p.pre) {
            p.pre = run;
            p.pre_at = pos + (uint32_t)k + 1u;
        }
        if (in && run <= lo) {
            lo = run;
            lo_at = pos + (uint32_t)k + 1u;
        }
    }
    p.sum = run;
    p.suf = run - lo;
    p.suf_at = lo_at;
    return p;
}

__global__ void __launch_bounds__(kEndtrimThreads) k_endtrim_spans(const SpanArgs a) {
    __shared__ uint32_t tab[256];
    tab[threadIdx.x] = c_endtrim_table[threadIdx.x];
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t n_waves = gridDim.x * kEndtrimWaves;
    const uint32_t total = a.seg_start[a.n_reads];
    const u32x4 zero = {0u, 0u, 0u, 0u};

    for (uint32_t sp = blockIdx.x * kEndtrimWaves + wave; sp < total; sp += n_waves) {
        const uint32_t lo = span_of(a.seg_start, a.n_reads, sp);
        const uint32_t read = a.order ? a.order[lo] : lo;
        const uint32_t len = (uint32_t)a.lengths[read];  // at least 1: the read has a span
        const uint32_t first_sp = a.seg_start[lo];
        const uint32_t s0 = (sp - first_sp) * (uint32_t)kSpan;
        const uint32_t s1 = min(len, s0 + (uint32_t)kSpan);  // this span: the bases [s0, s1), s0 < s1
        const uint8_t *base = a.plane + a.offsets[read];      // 16-byte aligned, and s0 is a multiple of 16

        Piece acc = endtrim::empty_at(s0);
        u32x4 nxt = s0 + lane * kLaneBases < s1 ? *(const u32x4 *)(base + s0 + lane * kLaneBases) : zero;
        for (uint32_t p0 = s0; p0 < s1; p0 += kStepBases) {
            const u32x4 cur = nxt;
            const uint32_t pos = p0 + lane * kLaneBases, pn = pos + kStepBases;
            nxt = pn < s1 ? *(const u32x4 *)(base + pn) : zero;  // (the next step's bytes are on their way during this one)
            Piece p;
            if (p0 + kStepBases <= s1) p = lane_piece<false>(cur, tab, pos, s1, a.t);  // (wave-uniform: a whole step)
            else p = lane_piece<true>(cur, tab, pos, s1, a.t);
            acc = endtrim::combine(acc, wave_combine(p, lane));  // (lane 0's is the span's)
        }
        if (lane == 0) {
            if (a.seg_start[lo + 1] - first_sp == 1u) {
                a.cuts[2ull * read] = acc.pre_at;
                a.cuts[2ull * read + 1] = len - acc.suf_at;
            } else if (sp < a.max_partials) {
                a.partials[sp] = acc;
            }
        }
    }
}

__global__ void __launch_bounds__(256) k_endtrim_reads(const SpanArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t r64 = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r64 >= a.n_reads) return;
    const uint32_t r = (uint32_t)r64;
    const uint32_t read = a.order ? a.order[r] : r;
    const uint32_t first_sp = a.seg_start[r], n_sp = a.seg_start[r + 1] - first_sp;
    if (n_sp == 1u) return;  // (k_endtrim_spans wrote its cuts)
    if (n_sp == 0u) {        // no base
        if (lane == 0) {
            a.cuts[2ull * read] = 0u;
            a.cuts[2ull * read + 1] = 0u;
        }
        return;
    }
    const uint32_t len = (uint32_t)a.lengths[read];
    const uint32_t per = (n_sp + 63u) / 64u;
    const uint32_t i0 = min(lane * per, n_sp), i1 = min(i0 + per, n_sp);  // this lane: the spans [i0, i1) of the read
    Piece p = endtrim::empty_at(i0 < n_sp ? i0 * (uint32_t)kSpan : len);
    for (uint32_t i = i0; i < i1; ++i)
        if (first_sp + i < a.max_partials) p = endtrim::combine(p, a.partials[first_sp + i]);
    p = wave_combine(p, lane);
    if (lane == 0) {
        a.cuts[2ull * read] = p.pre_at;
        a.cuts[2ull * read + 1] = len - p.suf_at;
    }
}

// per read: children (0 or 1), first and last; n_child[n_reads] = 0 (the scan's last entry is the total)
__global__ void __launch_bounds__(256) k_endtrim_children(uint64_t n_reads, const int32_t *lengths, const uint32_t *cuts, int64_t *n_child,
                                                          int32_t *first, int32_t *last) {
    const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (r > n_reads) return;
    if (r == n_reads) {
        n_child[r] = 0;
        return;
    }
    const int32_t l = lengths[r];
    int32_t f, e;
    n_child[r] = endtrim::child_of(cuts[2 * r], cuts[2 * r + 1], l < 0 ? 0 : l, &f, &e);
    first[r] = f;
    last[r] = e;
}

__global__ void __launch_bounds__(256) k_endtrim_emit(uint64_t n_reads, const uint64_t *child_offsets, const int32_t *first, const int32_t *last,
                                                      uint64_t capacity, int32_t *child_ranges, uint32_t *child_parent) {
    const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n_reads) return;
    const uint64_t at = child_offsets[r];
    if (child_offsets[r + 1] == at || at >= capacity) return;
    child_ranges[2 * at] = first[r];
    child_ranges[2 * at + 1] = last[r];
    child_parent[at] = (uint32_t)r;
}

}  // namespace

extern "C" uint32_t flx_endtrim_span(void) { return (uint32_t)kSpan; }

extern "C" int flx_endtrim_cuts_dev(flx_ctx *ctx, const void *d_plane, uint64_t plane_bytes, const void *d_offsets, const void *d_lengths,
                                    const void *d_order, uint64_t n_reads, uint64_t t, uint32_t *d_cuts) {
    if (!ctx) return FLX_ERR_INVALID;
    if (t > 0xffffffffull) return flx_fail(ctx, FLX_ERR_INVALID, "flx_endtrim_cuts: t must be below 2^32");
    if (n_reads > 0x7fffffffull) return flx_fail(ctx, FLX_ERR_INVALID, "at most 2^31-1 reads per batch");
    if (plane_bytes & 15) return flx_fail(ctx, FLX_ERR_INVALID, "plane_bytes must be a multiple of 16");
    if (n_reads == 0) return FLX_OK;
    if (!d_plane || !d_offsets || !d_lengths || !d_cuts) return flx_fail(ctx, FLX_ERR_INVALID, "plane/offsets/lengths/cuts must not be NULL");
    // (a read of L bases has ceil(L / span) spans and the reads share no byte of the plane)
    const uint64_t max_partials = plane_bytes / (uint64_t)kSpan + n_reads;
    if (max_partials > 0xffffffffull) return flx_fail(ctx, FLX_ERR_INVALID, "too many spans in one batch");
    FLX_HIP(ctx, hipSetDevice(ctx->device));
    void *partials = nullptr;
    FLX_CHECK(flx_workspace(ctx, 3, max_partials * sizeof(Piece), &partials));
    flx_time_scope timed(ctx, "flx_endtrim");
    SpanArgs a;
    memset(&a, 0, sizeof a);
    uint32_t *seg_start = nullptr;
    FLX_CHECK(flx_screen_segment_table(ctx, (const int32_t *)d_lengths, (const uint32_t *)d_order, n_reads, 1, &seg_start, (uint32_t)kSpan));
    a.plane = (const uint8_t *)d_plane;
    a.offsets = (const uint64_t *)d_offsets;
    a.lengths = (const int32_t *)d_lengths;
    a.order = (const uint32_t *)d_order;
    a.n_reads = (uint32_t)n_reads;
    a.seg_start = seg_start;
    a.t = t;
    a.partials = (Piece *)partials;
    a.max_partials = (uint32_t)max_partials;
    a.cuts = d_cuts;
    const unsigned n_cu = (unsigned)ctx->prop.multiProcessorCount;
    hipLaunchKernelGGL(k_endtrim_spans, dim3(kEndtrimBlocksPerCU * n_cu), dim3(kEndtrimThreads), 0, ctx->stream, a);
    FLX_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_endtrim_reads, dim3((unsigned)((n_reads + 3) / 4)), dim3(256), 0, ctx->stream, a);
    FLX_HIP(ctx, hipGetLastError());
    timed.end();
    return FLX_OK;
}

// the host-array form: everything staged through device buffers of the call's own
extern "C" int flx_endtrim_cuts(flx_ctx *ctx, const uint8_t *plane, uint64_t plane_bytes, const uint64_t *offsets, const int32_t *lengths,
                                const uint32_t *order, uint64_t n_reads, uint64_t t, uint32_t *cuts) {
    if (!ctx) return FLX_ERR_INVALID;
    if (t > 0xffffffffull) return flx_fail(ctx, FLX_ERR_INVALID, "flx_endtrim_cuts: t must be below 2^32");
    if (n_reads > 0x7fffffffull) return flx_fail(ctx, FLX_ERR_INVALID, "at most 2^31-1 reads per batch");
    if (plane_bytes & 15) return flx_fail(ctx, FLX_ERR_INVALID, "plane_bytes must be a multiple of 16");
    if (n_reads == 0) return FLX_OK;
    if (!plane || !offsets || !lengths || !cuts) return flx_fail(ctx, FLX_ERR_INVALID, "plane/offsets/lengths/cuts must not be NULL");
    FLX_CHECK(flx_check_reads(ctx, plane_bytes, offsets, lengths, order, n_reads));  // (every read's cuts are written exactly once)
    FLX_HIP(ctx, hipSetDevice(ctx->device));
    flx_dbuf d_plane, d_off, d_len, d_ord, d_cuts;
    FLX_CHECK(flx_dalloc(ctx, d_plane, plane_bytes ? plane_bytes : 16));
    FLX_CHECK(flx_dalloc(ctx, d_off, n_reads * 8));
    FLX_CHECK(flx_dalloc(ctx, d_len, n_reads * 4));
    FLX_CHECK(flx_dalloc(ctx, d_cuts, n_reads * 8));
    if (plane_bytes) FLX_HIP(ctx, hipMemcpyAsync(d_plane.p, plane, plane_bytes, hipMemcpyHostToDevice, ctx->stream));
    FLX_HIP(ctx, hipMemcpyAsync(d_off.p, offsets, n_reads * 8, hipMemcpyHostToDevice, ctx->stream));
    FLX_HIP(ctx, hipMemcpyAsync(d_len.p, lengths, n_reads * 4, hipMemcpyHostToDevice, ctx->stream));
    if (order) {
        FLX_CHECK(flx_dalloc(ctx, d_ord, n_reads * 4));
        FLX_HIP(ctx, hipMemcpyAsync(d_ord.p, order, n_reads * 4, hipMemcpyHostToDevice, ctx->stream));
    }
    // (a pattern no cut can be: a kernel that wrote nothing must not hand back an earlier call's answers — score_api.hip)
    FLX_HIP(ctx, hipMemsetAsync(d_cuts.p, 0xA5, n_reads * 8, ctx->stream));
    FLX_CHECK(flx_endtrim_cuts_dev(ctx, d_plane.p, plane_bytes, d_off.p, d_len.p, order ? d_ord.p : nullptr, n_reads, t, d_cuts.as<uint32_t>()));
    FLX_HIP(ctx, hipMemcpyAsync(cuts, d_cuts.p, n_reads * 8, hipMemcpyDeviceToHost, ctx->stream));
    FLX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return FLX_OK;
}

// flx_score_batch_endtrim_dev; the cuts stay in d_cuts_out when that is not NULL (pipeline.hip)
int flx_endtrim_score_dev(flx_ctx *ctx, const void *d_plane, uint64_t plane_bytes, const void *d_offsets, const void *d_lengths, const void *d_order,
                          uint64_t n_reads, const flx_params *params, uint64_t t, flx_scores *out, uint32_t *d_cuts_out) {
    if (!ctx) return FLX_ERR_INVALID;
    if (!params || !out) return flx_fail(ctx, FLX_ERR_INVALID, "params/out must not be NULL");
    if (t > 0xffffffffull) return flx_fail(ctx, FLX_ERR_INVALID, "flx_score_batch_endtrim: t must be below 2^32");
    if (n_reads > 0x7fffffffull) return flx_fail(ctx, FLX_ERR_INVALID, "at most 2^31-1 reads per batch");
    if (plane_bytes & 15) return flx_fail(ctx, FLX_ERR_INVALID, "plane_bytes must be a multiple of 16");
    if (n_reads && (!out->mean_q || !out->window_q || !out->passed))
        return flx_fail(ctx, FLX_ERR_INVALID, "mean_q/window_q/passed outputs are required");
    if (params->window_size <= 0) return flx_fail(ctx, FLX_ERR_INVALID, "window_size must be positive");
    if (params->trim || params->split_set) return flx_fail(ctx, FLX_ERR_INVALID, "trim/split need a k-mer set: not with trim_ends_q");
    if (!out->child_offsets) return flx_fail(ctx, FLX_ERR_INVALID, "trim_ends_q requested but child_offsets is NULL");
    out->n_children = 0;
    if (n_reads == 0) return FLX_OK;
    if (!d_plane) return flx_fail(ctx, FLX_ERR_INVALID, "the quality plane must not be NULL");
    FLX_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
    char *wp = nullptr;
    auto carve = [&](size_t bytes) { void *p = wp; wp += up(bytes); return p; };

    // ---- per-read arrays (workspace 0) ----
    const size_t scan_ws = flx_radix_sort_workspace(n_reads + 1);
    void *small = nullptr;
    FLX_CHECK(flx_workspace(ctx, 0, up((n_reads + 1) * 8) + 2 * up(n_reads * 4) + up(n_reads * 8) + up(scan_ws), &small));
    wp = (char *)small;
    int64_t *d_nchild = (int64_t *)carve((n_reads + 1) * 8);
    int32_t *d_first_tmp = (int32_t *)carve(n_reads * 4), *d_last_tmp = (int32_t *)carve(n_reads * 4);
    uint32_t *d_cuts = (uint32_t *)carve(n_reads * 8);
    if (d_cuts_out) d_cuts = d_cuts_out;
    void *d_scanws = carve(scan_ws);
    int32_t *first = out->first ? out->first : d_first_tmp, *last = out->last ? out->last : d_last_tmp;

    // ---- the cuts -> child_offsets ----
    FLX_CHECK(flx_endtrim_cuts_dev(ctx, d_plane, plane_bytes, d_offsets, d_lengths, d_order, n_reads, t, d_cuts));
    const unsigned grid = (unsigned)((n_reads + 1 + 255) / 256);
    hipLaunchKernelGGL(k_endtrim_children, dim3(grid), dim3(256), 0, st, n_reads, (const int32_t *)d_lengths, (const uint32_t *)d_cuts, d_nchild, first,
                       last);
    FLX_HIP(ctx, hipGetLastError());
    FLX_CHECK(flx_exclusive_scan_i64(ctx, n_reads + 1, d_nchild, (int64_t *)out->child_offsets, d_scanws, scan_ws));
    int64_t total = 0;
    FLX_HIP(ctx, hipMemcpyAsync(&total, (int64_t *)out->child_offsets + n_reads, 8, hipMemcpyDeviceToHost, st));
    FLX_HIP(ctx, hipStreamSynchronize(st));
    out->n_children = (uint64_t)total;
    if ((uint64_t)total > out->child_capacity)
        return flx_fail(ctx, FLX_ERR_CAPACITY, "child outputs need room for %lld children (capacity %llu)", (long long)total,
                        (unsigned long long)out->child_capacity);
    const uint64_t nc = (uint64_t)total;
    if (nc && (!out->child_ranges || !out->child_mean_q || !out->child_window_q || !out->child_passed))
        return flx_fail(ctx, FLX_ERR_INVALID, "child outputs are NULL");

    return flx_phred_children(ctx, d_plane, plane_bytes, d_offsets, d_lengths, d_order, n_reads, params, out, first, nc, [&](uint32_t *d_parent) {
        hipLaunchKernelGGL(k_endtrim_emit, dim3(grid), dim3(256), 0, st, n_reads, (const uint64_t *)out->child_offsets, (const int32_t *)first,
                           (const int32_t *)last, nc, out->child_ranges, d_parent);
        FLX_HIP(ctx, hipGetLastError());
        return (int)FLX_OK;
    });
}

extern "C" int flx_score_batch_endtrim_dev(flx_ctx *ctx, const void *d_plane, uint64_t plane_bytes, const void *d_offsets, const void *d_lengths,
                                           const void *d_order, uint64_t n_reads, const flx_params *params, uint64_t t, flx_scores *out) {
    return flx_endtrim_score_dev(ctx, d_plane, plane_bytes, d_offsets, d_lengths, d_order, n_reads, params, t, out, nullptr);
}
