// adapters_split.hip — --split_adapters: chimeric reads are split at the adapters inside them (adapters.h has the definition and the
// argument why a read may be cut into pieces that are searched independently).
//
// The same approximate matching as at the read ends (adapters.hip), but over every base of every read: compute-bound, and a read
// of any length spreads over the chip by itself.
//
//   pieces           a read of L bases has ceil(L / S) pieces of S = 1024 bases.  k_adapter_piece_counts writes the count per read in
//                    processing order, an exclusive scan turns the counts into the piece table: piece g belongs to the read i with
//                    start[i] <= g < start[i + 1] (a binary search per piece), and is its piece g - start[i].
//   k_adapter_marks  the work item is a (piece, pattern) pair, pattern-minor, so the lanes of a wave mostly share one text.  A
//                    workgroup takes `ppb` consecutive pieces and stages their texts once in LDS: kWarmup = 96 bases in front of the
//                    piece, then its S bases, one byte a base, already folded to the 2-bit code or kNoBase.  Staging reads the bytes
//                    [offset, offset + L) of a read and no other.  A lane walks the column of its pattern from the start of the
//                    warm-up (a fresh column; the true one where the piece is the read's first) to the end of the piece with
//                    column_advance (column_step without the minimum's bookkeeping) and four compare-and-selects per base: no table
//                    lookup, no dynamic register indexing, no scratch.
//                    Hit ends are only looked for inside the piece.  A lane keeps the current run of marked bases in two registers
//                    and flushes a finished run into the mark bitmap with atomicOr on 32-bit words: hits are rare, atomics are rare.
//                    The grid is sized from plane_bytes (no host round trip for the piece total) and strides over the groups of
//                    pieces, so any total is covered.
//   mark bitmap      one bit per byte of the plane: bit offset + i is base i of the read at `offset`; zeroed per call.
//   k_adapter_split  one wave per read, 64 lanes x 32 bases a step over the bitmap words between s and e: every word gives the bits
//                    where a child starts and where one ends (adapters::child_edges), a wave scan of both counts numbers them, and
//                    the k-th start and the k-th end are one child.  The count pass writes n_child, first and last; after the
//                    exclusive scan the emit pass writes child_ranges and child_parent and leaves a read without children at once.
//                    Everything behind that is flx_phred_children (qsplit.hip), unchanged.
#include <algorithm>

#include "adapters_internal.h"
#include "rank_internal.h"

using adapters::Pattern;

namespace {

constexpr int kThreads = 256;
constexpr int kPieceBases = 1024;                               // S
constexpr int kPieceStride = adapters::kWarmup + kPieceBases;   // bytes of LDS per piece
constexpr int kMaxPieces = 28;                                  // pieces per workgroup at most: 30.6 KiB of texts, five workgroups a CU
constexpr int kItemsPerGroup = 1024;                            // (piece, pattern) pairs a workgroup aims for: four rounds of its lanes
constexpr int kMaxGroups = 8192;                                // workgroups of one launch at most; they stride over the rest
constexpr int kSplitWaves = 4;                                  // reads per workgroup of k_adapter_split

static_assert(adapters::kWarmup % 4 == 0 && kPieceBases % 4 == 0, "the texts are read four bases a dword");
static_assert(adapters::kWarmup >= adapters::kMaxBases + adapters::kMaxBases * adapters::kMaxErrors / 100, "the warm-up covers m + k2");

struct MarkArgs {
    const uint8_t *plane;
    const uint64_t *offsets;
    const int32_t *lengths;
    const uint32_t *order;
    uint64_t n_reads;
    const int64_t *piece_start;  // [n_reads + 1], by processing order; the last entry is the number of pieces
    const Pattern *patterns;
    uint32_t n_patterns;
    uint32_t e2;   // --adapter_split_errors
    uint32_t ppb;  // pieces per workgroup
    uint32_t *marks;
};

// pieces per read, in processing order; cnt[n_reads] = 0 (the scan's last entry is the total)
__global__ void __launch_bounds__(256) k_adapter_piece_counts(uint64_t n_reads, const int32_t *lengths, const uint32_t *order, int64_t *cnt) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i > n_reads) return;
    int64_t c = 0;
    if (i < n_reads) {
        const int32_t l = lengths[order ? order[i] : (uint32_t)i];
        c = l > 0 ? ((int64_t)l + kPieceBases - 1) / kPieceBases : 0;
    }
    cnt[i] = c;
}

__global__ void __launch_bounds__(kThreads) k_adapter_marks(const MarkArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t s_text[];  // [ppb][kPieceStride]
    __shared__ int32_t s_a[kMaxPieces];                                // the piece's first base in its read
    __shared__ int32_t s_nb[kMaxPieces];                               // its bases (0: nothing to do)
    __shared__ uint64_t s_off[kMaxPieces];                             // the read's offset in the plane
    const uint64_t total = (uint64_t)a.piece_start[a.n_reads];

    for (uint64_t g0 = (uint64_t)blockIdx.x * a.ppb; g0 < total; g0 += (uint64_t)gridDim.x * a.ppb) {  // (the same for every lane)
        if (threadIdx.x < a.ppb) {
            const uint32_t le = threadIdx.x;
            const uint64_t g = g0 + le;
            int32_t pa = 0, nb = 0;
            uint64_t off = 0;
            if (g < total) {
                uint64_t lo = 0, hi = a.n_reads;  // the read i with piece_start[i] <= g < piece_start[i + 1]
                while (lo < hi) {
                    const uint64_t mid = (lo + hi) >> 1;
                    if ((uint64_t)a.piece_start[mid + 1] <= g) lo = mid + 1;
                    else hi = mid;
                }
                const uint32_t read = a.order ? a.order[lo] : (uint32_t)lo;
                const int64_t l = a.lengths[read];
                const int64_t first = (int64_t)(g - (uint64_t)a.piece_start[lo]) * kPieceBases;
                const int64_t end = first + kPieceBases < l ? first + kPieceBases : l;
                pa = (int32_t)first;
                nb = end > first ? (int32_t)(end - first) : 0;
                off = a.offsets[read];
            }
            s_a[le] = pa;
            s_nb[le] = nb;
            s_off[le] = off;
        }
        __syncthreads();

        // the texts: byte i of a piece's text is base a - kWarmup + i of its read; only bases [0, a + nb) are read
        constexpr uint32_t kDwords = kPieceStride / 4;
        for (uint32_t q = threadIdx.x; q < a.ppb * kDwords; q += kThreads) {
            const uint32_t le = q / kDwords, i = (q - le * kDwords) * 4;
            const int64_t pos = (int64_t)s_a[le] - adapters::kWarmup + i, end = (int64_t)s_a[le] + s_nb[le];
            uint32_t w = adapters::kNoBase * 0x01010101u;
            if (s_nb[le] > 0 && pos + 4 > 0 && pos < end) {
                const uint8_t *src = a.plane + s_off[le] + pos;
                w = 0;
                if (pos >= 0 && pos + 4 <= end) {  // (offsets are multiples of 16 and pos of 4: an aligned dword inside the read)
                    const uint32_t four = *(const uint32_t *)src;
#pragma unroll
                    for (int b = 0; b < 4; ++b) w |= adapters::code_of((uint8_t)(four >> (8 * b))) << (8 * b);
                } else {
#pragma unroll
                    for (int b = 0; b < 4; ++b) {
                        const bool in = pos + b >= 0 && pos + b < end;
                        w |= (in ? adapters::code_of(src[b]) : adapters::kNoBase) << (8 * b);
                    }
                }
            }
            ((uint32_t *)s_text)[q] = w;
        }
        __syncthreads();

        const uint32_t items = a.ppb * a.n_patterns;
        for (uint32_t it = threadIdx.x; it < items; it += kThreads) {
            const uint32_t le = it / a.n_patterns, p = it - le * a.n_patterns;
            const int32_t nb = s_nb[le];
            if (nb == 0) continue;
            const int32_t pa = s_a[le];
            const uint64_t off = s_off[le];
            const Pattern *pat = a.patterns + p;
            const uint64_t peq0 = pat->peq_head[0], peq1 = pat->peq_head[1], peq2 = pat->peq_head[2], peq3 = pat->peq_head[3];
            const int32_t m = (int32_t)pat->m, k2 = (int32_t)adapters::edits_allowed(pat->m, a.e2);
            const uint64_t top = 1ull << (m - 1);
            adapters::Column col;
            adapters::column_start(&col, (uint32_t)m);
            adapters::MarkRun run;
            uint32_t *marks = a.marks;
            auto flush = [&](int32_t lo, int32_t hi) {  // the bits [off + lo, off + hi), all inside the read's own bits
                const uint64_t b0 = off + (uint64_t)lo, b1 = off + (uint64_t)hi - 1;
                for (uint64_t w = b0 >> 5; w <= b1 >> 5; ++w) {
                    uint32_t mask = ~0u;
                    if (w == b0 >> 5) mask &= ~0u << (b0 & 31);
                    if (w == b1 >> 5) mask &= ~0u >> (31 - (b1 & 31));
                    atomicOr(&marks[w], mask);
                }
            };
            auto step = [&](uint32_t code) {
                uint64_t eq = 0;
                eq = code == 0u ? peq0 : eq;
                eq = code == 1u ? peq1 : eq;
                eq = code == 2u ? peq2 : eq;
                eq = code == 3u ? peq3 : eq;
                adapters::column_advance(&col, eq, top);
            };
            const uint32_t *text = (const uint32_t *)(s_text + le * kPieceStride);
            // the warm-up (the read's first piece has none: its column is the true one from the start)
            for (int32_t i0 = pa ? 0 : adapters::kWarmup; i0 < adapters::kWarmup; i0 += 4) {
                const uint32_t four = text[i0 >> 2];
#pragma unroll
                for (int b = 0; b < 4; ++b) step((four >> (8 * b)) & 0xffu);
            }
            // the piece: text byte kWarmup + i is base pa + i, whose hit end is j = pa + i + 1
            const int32_t whole = nb & ~3;
            for (int32_t i0 = 0; i0 < whole; i0 += 4) {
                const uint32_t four = text[(adapters::kWarmup + i0) >> 2];
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    step((four >> (8 * b)) & 0xffu);
                    if (col.score <= k2) adapters::mark_hit(&run, pa + i0 + b + 1, m, flush);
                }
            }
            if (whole < nb) {
                const uint32_t four = text[(adapters::kWarmup + whole) >> 2];
                for (int b = 0; whole + b < nb; ++b) {
                    step((four >> (8 * b)) & 0xffu);
                    if (col.score <= k2) adapters::mark_hit(&run, pa + whole + b + 1, m, flush);
                }
            }
            adapters::mark_end(&run, flush);
        }
        __syncthreads();  // (the next round's staging overwrites the texts)
    }
}

struct SplitArgs {
    const uint64_t *offsets;
    const int32_t *lengths;
    const uint32_t *keys;
    const uint32_t *marks;
    uint64_t n_reads;
    // count pass
    int64_t *n_child;  // [n_reads + 1]
    int32_t *first, *last;
    // emit pass
    const uint64_t *child_offsets;
    int32_t *child_ranges;
    uint32_t *child_parent;
    uint64_t capacity;
};

__device__ __forceinline__ uint32_t wave_scan_add(uint32_t v, int lane) {  // inclusive
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t u = __shfl_up(v, (unsigned)o, 64);
        if (lane >= o) v += u;
    }
    return v;
}

template <bool EMIT>
__global__ void __launch_bounds__(kSplitWaves * 64) k_adapter_split(const SplitArgs a) {
    const int lane = threadIdx.x & 63;
    const uint64_t r = (uint64_t)blockIdx.x * kSplitWaves + (threadIdx.x >> 6);
    if (r > a.n_reads) return;
    if (r == a.n_reads) {
        if (!EMIT && lane == 0) a.n_child[r] = 0;  // (the scan's last entry is the total)
        return;
    }
    const uint64_t out_base = EMIT ? a.child_offsets[r] : 0;
    if (EMIT && a.child_offsets[r + 1] == out_base) return;  // (the count pass found no child: nothing to write)
    const int64_t l = a.lengths[r] < 0 ? 0 : a.lengths[r];
    const uint32_t kh = a.keys[2 * r], kt = a.keys[2 * r + 1];
    const bool end_hit = (kh | kt) != 0u;
    int64_t s, e;
    if (!adapters::kept_range(kh, kt, l, &s, &e)) {
        if (!EMIT && lane == 0) {
            int32_t f, t;
            a.n_child[r] = adapters::split_summary(end_hit, false, 0, l, -1, -1, &f, &t);
            a.first[r] = f;
            a.last[r] = t;
        }
        return;
    }
    const uint64_t off = a.offsets[r], b0 = off + (uint64_t)s, b1 = off + (uint64_t)e;  // the bits [b0, b1) of the bitmap, b0 < b1
    const uint64_t w_first = b0 >> 5, w_last = (b1 - 1) >> 5;
    uint32_t carry = 0, any_mark = 0;
    uint64_t n_start = 0, n_end = 0;
    int32_t my_first = 0x7fffffff, my_last = -1;

    for (uint64_t w0 = w_first; w0 <= (b1 >> 5); w0 += 64) {  // (up to the word of bit b1: a child that reaches e ends there)
        const uint64_t w = w0 + (uint64_t)lane;
        uint32_t free_bits = 0;
        if (w <= w_last) {
            uint32_t valid = ~0u;
            if (w == w_first) valid &= ~0u << (b0 & 31);
            if (w == w_last) valid &= ~0u >> (31 - ((b1 - 1) & 31));
            const uint32_t m = a.marks[w];
            free_bits = ~m & valid;
            any_mark |= m & valid;
        }
        uint32_t before = __shfl_up(free_bits >> 31, 1u, 64);
        if (lane == 0) before = carry;
        carry = __shfl(free_bits >> 31, 63, 64);
        uint32_t starts, ends;
        adapters::child_edges(free_bits, before, &starts, &ends);
        if (w > (b1 >> 5)) ends = 0;  // (a word behind the walk)
        if (__ballot((starts | ends) != 0u) == 0) continue;  // (wave-uniform)

        const uint32_t cnt = (uint32_t)__popc(starts) | ((uint32_t)__popc(ends) << 16);  // at most 16 each a word, 1024 a step
        const uint32_t scan = wave_scan_add(cnt, lane);
        const uint32_t all = __shfl(scan, 63, 64);
        const int64_t bit0 = (int64_t)(w << 5) - (int64_t)off;  // the word's first bit as a base of the read
        if (EMIT) {
            uint64_t k = out_base + n_start + ((scan - cnt) & 0xffffu);
            for (uint32_t x = starts; x; x &= x - 1, ++k) {
                if (k < a.capacity) {
                    a.child_ranges[2 * k] = (int32_t)(bit0 + (__ffs((int)x) - 1));
                    a.child_parent[k] = (uint32_t)r;
                }
            }
            k = out_base + n_end + ((scan - cnt) >> 16);
            for (uint32_t x = ends; x; x &= x - 1, ++k)
                if (k < a.capacity) a.child_ranges[2 * k + 1] = (int32_t)(bit0 + (__ffs((int)x) - 1));
        } else {
            if (starts) my_first = min(my_first, (int32_t)(bit0 + (__ffs((int)starts) - 1)));
            if (ends) my_last = max(my_last, (int32_t)(bit0 + (31 - __clz((int)ends))));
        }
        n_start += all & 0xffffu;
        n_end += all >> 16;
    }

    if (!EMIT) {
        for (int o = 32; o; o >>= 1) {
            my_first = min(my_first, __shfl_xor(my_first, o, 64));
            my_last = max(my_last, __shfl_xor(my_last, o, 64));
            any_mark |= __shfl_xor(any_mark, o, 64);
        }
        if (lane == 0) {
            int32_t f, t;
            a.n_child[r] = adapters::split_summary(end_hit, any_mark != 0u, (int64_t)n_start, l, my_first, my_last, &f, &t);
            a.first[r] = f;
            a.last[r] = t;
        }
    }
}

size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }

}  // namespace

size_t flx_adapter_marks_scratch(uint64_t n_reads) { return 2 * up256((n_reads + 1) * 8) + up256(flx_radix_sort_workspace(n_reads + 1)); }

int flx_adapter_marks_launch(flx_ctx *ctx, flx_adapters *ad, int split_errors_percent, const void *d_plane, uint64_t plane_bytes,
                             const void *d_offsets, const void *d_lengths, const void *d_order, uint64_t n_reads, uint32_t *d_marks, void *d_scratch) {
    hipStream_t st = ctx->stream;
    MarkArgs a;
    memset(&a, 0, sizeof a);
    FLX_CHECK(flx_adapters_table(ctx, ad, &a.patterns));
    char *wp = (char *)d_scratch;
    int64_t *d_cnt = (int64_t *)wp;
    wp += up256((n_reads + 1) * 8);
    int64_t *d_start = (int64_t *)wp;
    wp += up256((n_reads + 1) * 8);
    const size_t scan_ws = flx_radix_sort_workspace(n_reads + 1);
    a.plane = (const uint8_t *)d_plane;
    a.offsets = (const uint64_t *)d_offsets;
    a.lengths = (const int32_t *)d_lengths;
    a.order = (const uint32_t *)d_order;
    a.n_reads = n_reads;
    a.piece_start = d_start;
    a.n_patterns = (uint32_t)ad->patterns.size();
    a.e2 = (uint32_t)split_errors_percent;
    a.ppb = std::max(1u, std::min((uint32_t)kItemsPerGroup / a.n_patterns, (uint32_t)kMaxPieces));
    a.marks = d_marks;
    // reads that do not overlap in the plane have at most plane_bytes / S + n_reads pieces; more than that (or more than kMaxGroups
    // workgroups' worth) is covered by the kernel's stride
    const uint64_t bound = plane_bytes / kPieceBases + n_reads;
    const uint64_t groups = std::max<uint64_t>(1, std::min<uint64_t>((bound + a.ppb - 1) / a.ppb, kMaxGroups));
    flx_time_scope timed(ctx, "flx_adapter_marks");
    FLX_HIP(ctx, hipMemsetAsync(d_marks, 0, adapters::mark_words(plane_bytes) * 4, st));
    hipLaunchKernelGGL(k_adapter_piece_counts, dim3((unsigned)((n_reads + 1 + 255) / 256)), dim3(256), 0, st, n_reads, (const int32_t *)d_lengths,
                       (const uint32_t *)d_order, d_cnt);
    FLX_HIP(ctx, hipGetLastError());
    FLX_CHECK(flx_exclusive_scan_i64(ctx, n_reads + 1, d_cnt, d_start, wp, scan_ws));
    hipLaunchKernelGGL(k_adapter_marks, dim3((unsigned)groups), dim3(kThreads), (size_t)a.ppb * kPieceStride, st, a);
    FLX_HIP(ctx, hipGetLastError());
    timed.end();
    return FLX_OK;
}

int flx_adapter_split_launch(flx_ctx *ctx, bool emit, uint64_t n_reads, const void *d_offsets, const void *d_lengths, const uint32_t *d_keys,
                             const uint32_t *d_marks, int64_t *d_nchild, int32_t *d_first, int32_t *d_last, const uint64_t *d_child_offsets,
                             uint64_t capacity, int32_t *d_child_ranges, uint32_t *d_child_parent) {
    SplitArgs a;
    memset(&a, 0, sizeof a);
    a.offsets = (const uint64_t *)d_offsets;
    a.lengths = (const int32_t *)d_lengths;
    a.keys = d_keys;
    a.marks = d_marks;
    a.n_reads = n_reads;
    a.n_child = d_nchild;
    a.first = d_first;
    a.last = d_last;
    a.child_offsets = d_child_offsets;
    a.child_ranges = d_child_ranges;
    a.child_parent = d_child_parent;
    a.capacity = capacity;
    const unsigned grid = (unsigned)((n_reads + 1 + kSplitWaves - 1) / kSplitWaves);
    flx_time_scope timed(ctx, emit ? "flx_adapter_split.emit" : "flx_adapter_split.count");
    if (emit) hipLaunchKernelGGL(k_adapter_split<true>, dim3(grid), dim3(kSplitWaves * 64), 0, ctx->stream, a);
    else hipLaunchKernelGGL(k_adapter_split<false>, dim3(grid), dim3(kSplitWaves * 64), 0, ctx->stream, a);
    FLX_HIP(ctx, hipGetLastError());
    timed.end();
    return FLX_OK;
}

extern "C" int flx_adapters_set_split(flx_adapters *ad, int split_errors_percent) {
    if (!ad || split_errors_percent < -1 || split_errors_percent > adapters::kMaxErrors) return FLX_ERR_INVALID;
    ad->split_errors_percent = split_errors_percent;
    return FLX_OK;
}

extern "C" int flx_adapters_split(const flx_adapters *ad) { return ad ? ad->split_errors_percent : -1; }

extern "C" int flx_adapter_marks_dev(flx_ctx *ctx, flx_adapters *ad, const void *d_plane, uint64_t plane_bytes, const void *d_offsets,
                                     const void *d_lengths, const void *d_order, uint64_t n_reads, uint32_t *d_marks) {
    if (!ctx) return FLX_ERR_INVALID;
    if (!ad) return flx_fail(ctx, FLX_ERR_INVALID, "flx_adapter_marks: adapters must not be NULL");
    if (ad->split_errors_percent < 0) return flx_fail(ctx, FLX_ERR_INVALID, "flx_adapter_marks: the middle search is off (flx_adapters_set_split)");
    if (n_reads > 0x7fffffffull) return flx_fail(ctx, FLX_ERR_INVALID, "at most 2^31-1 reads per batch");
    if (plane_bytes & 15) return flx_fail(ctx, FLX_ERR_INVALID, "plane_bytes must be a multiple of 16");
    if (n_reads == 0) return FLX_OK;
    if (!d_plane || !d_offsets || !d_lengths || !d_marks) return flx_fail(ctx, FLX_ERR_INVALID, "plane/offsets/lengths/marks must not be NULL");
    FLX_HIP(ctx, hipSetDevice(ctx->device));
    void *scratch = nullptr;
    FLX_CHECK(flx_workspace(ctx, 0, flx_adapter_marks_scratch(n_reads), &scratch));
    return flx_adapter_marks_launch(ctx, ad, ad->split_errors_percent, d_plane, plane_bytes, d_offsets, d_lengths, d_order, n_reads, d_marks, scratch);
}

extern "C" int flx_adapter_marks(flx_ctx *ctx, flx_adapters *ad, const uint8_t *plane, uint64_t plane_bytes, const uint64_t *offsets,
                                 const int32_t *lengths, const uint32_t *order, uint64_t n_reads, uint32_t *marks) {
    if (!ctx) return FLX_ERR_INVALID;
    if (!ad) return flx_fail(ctx, FLX_ERR_INVALID, "flx_adapter_marks: adapters must not be NULL");
    if (ad->split_errors_percent < 0) return flx_fail(ctx, FLX_ERR_INVALID, "flx_adapter_marks: the middle search is off (flx_adapters_set_split)");
    if (n_reads > 0x7fffffffull) return flx_fail(ctx, FLX_ERR_INVALID, "at most 2^31-1 reads per batch");
    if (plane_bytes & 15) return flx_fail(ctx, FLX_ERR_INVALID, "plane_bytes must be a multiple of 16");
    if (n_reads == 0) return FLX_OK;
    if (!plane || !offsets || !lengths || !marks) return flx_fail(ctx, FLX_ERR_INVALID, "plane/offsets/lengths/marks must not be NULL");
    FLX_CHECK(flx_check_reads(ctx, plane_bytes, offsets, lengths, order, n_reads));
    FLX_HIP(ctx, hipSetDevice(ctx->device));
    const uint64_t mark_bytes = adapters::mark_words(plane_bytes) * 4;
    flx_dbuf d_plane, d_off, d_len, d_ord, d_marks;
    FLX_CHECK(flx_dalloc(ctx, d_plane, plane_bytes ? plane_bytes : 16));
    FLX_CHECK(flx_dalloc(ctx, d_off, n_reads * 8));
    FLX_CHECK(flx_dalloc(ctx, d_len, n_reads * 4));
    FLX_CHECK(flx_dalloc(ctx, d_marks, mark_bytes ? mark_bytes : 16));
    if (plane_bytes) FLX_HIP(ctx, hipMemcpyAsync(d_plane.p, plane, plane_bytes, hipMemcpyHostToDevice, ctx->stream));
    FLX_HIP(ctx, hipMemcpyAsync(d_off.p, offsets, n_reads * 8, hipMemcpyHostToDevice, ctx->stream));
    FLX_HIP(ctx, hipMemcpyAsync(d_len.p, lengths, n_reads * 4, hipMemcpyHostToDevice, ctx->stream));
    if (order) {
        FLX_CHECK(flx_dalloc(ctx, d_ord, n_reads * 4));
        FLX_HIP(ctx, hipMemcpyAsync(d_ord.p, order, n_reads * 4, hipMemcpyHostToDevice, ctx->stream));
    }
    FLX_CHECK(flx_adapter_marks_dev(ctx, ad, d_plane.p, plane_bytes, d_off.p, d_len.p, order ? d_ord.p : nullptr, n_reads, d_marks.as<uint32_t>()));
    if (mark_bytes) FLX_HIP(ctx, hipMemcpyAsync(marks, d_marks.p, mark_bytes, hipMemcpyDeviceToHost, ctx->stream));
    FLX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return FLX_OK;
}
