// cover_long.hip — the cooperative path of the coverage stage of k-mer mode: ultra-long reads covered as segments, one wave each.
//
// k_kmer_cover_q (cover_queue.hip) / k_kmer_cover_w (cover_wave.hip) give a read to ONE wave, which walks it span by span.  Inside a batch of 10^11 bases, longest
// first, that hides a 4 Mbp read; in a streamed chunk or an ultra-long dataset of a few Gbases the read is a serial tail many times
// the batch's own time.  Coverage is a pure function of the read and the set — base i is covered iff a member 16-mer starts in
// [i - 15, i] (src/read.cpp:43-58) — and the text, seed and diagonal machinery of the kernels only takes exact shortcuts to those
// answers, so a read can be cut anywhere as long as both sides see 15 bases of context: bit-identity needs no new argument.
//
// So a read of at least the threshold is left alone by the batch launch (CoverArgs::long_min) and cut into segments of `spans` spans
// (cover_segments.h).  A small kernel writes the SEGMENT TABLE — per segment the virtual read's plane offset, length and row offset,
// its emit range, and room for its count / first / last and its hand-over mark — and the same cover kernels run on that table as on
// a batch of reads (their SEGMENTS instantiations write and count the emit range only).  A reduce kernel then turns the segments'
// results into the read's.  The hand-over to the lane-diagonal kernel works per segment, with the marks of the table.
#include <cerrno>
#include <chrono>

#include "flx_internal.h"
#include "cover_common.h"

namespace {

constexpr size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }

// the table in the workspace: per segment, then per long read
struct SegLayout {
    size_t off, covoff, len, emit, cnt, fst, lst, redo, rid, base, end;
    explicit SegLayout(const CoverLongCounts &n) {
        const size_t G = (size_t)n.n_segs, R = (size_t)n.n_reads;
        size_t at = 0;
        auto take = [&](size_t bytes) { const size_t o = at; at += up256(bytes); return o; };
        off = take(G * 8);
        covoff = take(G * 8);
        len = take(G * 4);
        emit = take(G * 8);
        cnt = take(G * 4);
        fst = take(G * 4);
        lst = take(G * 4);
        redo = take(G);
        rid = take(R * 4);
        base = take(R * 8);
        end = at;
    }
};

struct SegTable {
    uint64_t *off, *covoff;
    int32_t *len;
    int2 *emit;
    int32_t *cnt, *fst, *lst;
    uint32_t *rid;   // [long reads] the read
    uint64_t *base;  // [long reads] its first segment
};

SegTable table_at(const SegLayout &l, char *w) {
    SegTable t;
    t.off = (uint64_t *)(w + l.off);
    t.covoff = (uint64_t *)(w + l.covoff);
    t.len = (int32_t *)(w + l.len);
    t.emit = (int2 *)(w + l.emit);
    t.cnt = (int32_t *)(w + l.cnt);
    t.fst = (int32_t *)(w + l.fst);
    t.lst = (int32_t *)(w + l.lst);
    t.rid = (uint32_t *)(w + l.rid);
    t.base = (uint64_t *)(w + l.base);
    return t;
}

// One thread per read of the batch; a long read takes its place among the long reads and its run of segments from two cursors
// (the order in which reads arrive does not matter: every segment writes words and results of its own) and writes its entries.
// Never more entries than k_cov_row_bytes counted: the same lengths, the same arithmetic.
__global__ void __launch_bounds__(256) k_cover_seg_table(uint64_t n, const int32_t *lengths, const uint64_t *offsets, const uint64_t *cov_off, int thr,
                                                         int seg_bases, CoverLongCounts *counts, CoverLongCounts limit, SegTable t) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int L = lengths[i];
    if (L < thr) return;
    const unsigned long long n_seg = (unsigned long long)flx_cover_seg_count(L, seg_bases);
    const unsigned long long r = atomicAdd(&counts->read_cursor, 1ull);
    const unsigned long long g0 = atomicAdd(&counts->seg_cursor, n_seg);
    if (r >= limit.n_reads || g0 + n_seg > limit.n_segs) return;  // (cannot happen: the counts are of these very lengths)
    t.rid[r] = (uint32_t)i;
    t.base[r] = g0;
    const uint64_t po = offsets[i], co = cov_off[i];
    for (unsigned long long k = 0; k < n_seg; ++k) {
        const CoverSeg s = flx_cover_seg(L, seg_bases, (long long)k);
        t.off[g0 + k] = po + (uint64_t)s.S;
        t.covoff[g0 + k] = co + (uint64_t)(s.S >> 3);
        t.len[g0 + k] = s.T - s.S;
        t.emit[g0 + k] = make_int2(s.emit_lo, s.emit_hi);
    }
}

// One thread per long read: count / first / last out of its segments' (cover_segments.h), and the words of its row behind its last
// base — a batch launch writes them as zeros with the read's last span, a segment writes the words of its emit range only.
__global__ void __launch_bounds__(256) k_cover_seg_reduce(uint64_t n_long, const int32_t *lengths, const uint64_t *cov_off, uint32_t *cov, int seg_bases,
                                                          SegTable t, int32_t *count, int32_t *first, int32_t *last) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_long) return;
    const uint32_t rid = t.rid[r];
    const int L = lengths[rid];
    const uint64_t g0 = t.base[r];
    const long long n_seg = flx_cover_seg_count(L, seg_bases);
    CoverTotals tot = {0, -1, -1};
    for (long long k = 0; k < n_seg; ++k) flx_cover_seg_add(tot, flx_cover_seg(L, seg_bases, k).S, t.cnt[g0 + k], t.fst[g0 + k], t.lst[g0 + k]);
    count[rid] = tot.count;
    first[rid] = tot.first;
    last[rid] = tot.last;
    uint32_t *row = cov + (cov_off[rid] >> 2);
    const int row_words = (((L + 7) / 8 + 15) & ~15) >> 2;
    for (int wd = (int)(((long long)L + 31) >> 5); wd < row_words; ++wd) row[wd] = 0;
}

double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// a switch that holds a non-negative integer; *set says whether it is there
int env_count(flx_ctx *ctx, const char *name, const char *value, const char *unit, unsigned long long *out, bool *set) {
    *set = value != nullptr;
    if (!value) return FLX_OK;
    char *end = nullptr;
    errno = 0;
    const unsigned long long v = strtoull(value, &end, 10);
    if (!*value || *end || errno || value[0] == '-' || value[0] == '+' || value[0] == ' ')
        return flx_fail(ctx, FLX_ERR_INVALID, "%s=%s: expected a non-negative integer (%s)", name, value, unit);
    *out = v;
    return FLX_OK;
}

}  // namespace

// ---------------------------------------------------------------------------------------------------- host side
// Threshold: the floor, doubled while the plane's bases per resident wave slot of the cover kernels (CUs x 4 SIMDs x
// FLX_COVER_WAVES_PER_EU) are at least twice as many — the argument of flx_kmer_long_threshold with wave slots in place of lanes: a
// read no longer than a wave's share of the batch finishes inside the batch's time anyway.  At 10^11 bases nothing leaves the batch.
// FLX_KMER_COVER_LONG_MIN: "0" = off, N = every read of at least N bases is covered in segments (tests).
// FLX_KMER_COVER_LONG_SPANS: spans per segment (tests, A/B).  32 spans — 32 Ki bases, 0.2 % of overlap — is a starting value.
#ifndef FLX_COVER_LONG_FLOOR
#define FLX_COVER_LONG_FLOOR (1 << 18)
#endif
#ifndef FLX_COVER_LONG_SPANS
#define FLX_COVER_LONG_SPANS 32
#endif
int flx_cover_long_threshold(flx_ctx *ctx, uint64_t plane_bytes, bool applies, CoverLong *cl) {
    *cl = CoverLong();
    unsigned long long thr = FLX_COVER_LONG_FLOOR, spans = FLX_COVER_LONG_SPANS;
    bool forced = false, spans_set = false;
    FLX_CHECK(env_count(ctx, "FLX_KMER_COVER_LONG_MIN", getenv("FLX_KMER_COVER_LONG_MIN"), "bases", &thr, &forced));
    FLX_CHECK(env_count(ctx, "FLX_KMER_COVER_LONG_SPANS", getenv("FLX_KMER_COVER_LONG_SPANS"), "spans of 1024 bases, 1 .. 1048576", &spans, &spans_set));
    if (spans_set && (spans == 0 || spans > (1ull << 20)))
        return flx_fail(ctx, FLX_ERR_INVALID, "FLX_KMER_COVER_LONG_SPANS=%llu: expected 1 .. 1048576 spans of 1024 bases", spans);
    if (forced && (thr == 0 || thr > 0x7fffffffull)) return FLX_OK;  // off (no read is that long)
    if (!applies) return FLX_OK;
    if (!forced) {
        const double per_wave = (double)plane_bytes / ((double)ctx->prop.multiProcessorCount * 4.0 * FLX_COVER_WAVES_PER_EU);
        while (thr < (1ull << 30) && (double)(thr * 2) <= per_wave) thr *= 2;
    }
    cl->on = true;
    cl->thr = (int)thr;
    cl->spans = (int)spans;
    return FLX_OK;
}

size_t flx_cover_long_workspace(const CoverLongCounts &n) { return SegLayout(n).end; }

int flx_cover_long_table(flx_ctx *ctx, CoverLong &cl, const CoverArgs &batch, CoverLongCounts *d_counts, void *work, size_t work_bytes, CoverArgs *seg) {
    const SegLayout lay(cl.n);
    if (!work || work_bytes < lay.end || cl.n.n_reads >= 0xffffffffull) return flx_fail(ctx, FLX_ERR_INVALID, "k-mer long cover: workspace");
    const SegTable t = table_at(lay, (char *)work);
    cl.t_start = now_s();
    hipLaunchKernelGGL(k_cover_seg_table, dim3((unsigned)((batch.n_reads + 255) / 256)), dim3(256), 0, ctx->stream, batch.n_reads, batch.lengths, batch.offsets,
                       batch.cov_off, cl.thr, cl.spans * 1024, d_counts, cl.n, t);
    FLX_HIP(ctx, hipGetLastError());
    *seg = batch;
    seg->offsets = t.off;
    seg->lengths = t.len;
    seg->order = nullptr;
    seg->n_reads = cl.n.n_segs;
    seg->cov_off = t.covoff;
    seg->count = t.cnt;
    seg->first = t.fst;
    seg->last = t.lst;
    seg->redo = (uint8_t *)work + lay.redo;
    seg->long_min = kCoverNoLong;
    seg->emit = t.emit;
    return FLX_OK;
}

int flx_cover_long_reduce(flx_ctx *ctx, const CoverLong &cl, const CoverArgs &batch, void *work) {
    const SegTable t = table_at(SegLayout(cl.n), (char *)work);
    hipLaunchKernelGGL(k_cover_seg_reduce, dim3((unsigned)((cl.n.n_reads + 255) / 256)), dim3(256), 0, ctx->stream, cl.n.n_reads, batch.lengths, batch.cov_off,
                       batch.cov, cl.spans * 1024, t, batch.count, batch.first, batch.last);
    FLX_HIP(ctx, hipGetLastError());
    return FLX_OK;
}

void flx_cover_long_report(const CoverLong &cl) {
    if (!getenv("FLX_API_TIMING") || cl.n.n_segs == 0) return;
    fprintf(stderr, "[flx_score_batch] %-22s %8.3f ms  (%llu reads of >= %d bases in %llu segments of %d spans)\n", "kmer long cover",
            (now_s() - cl.t_start) * 1e3, cl.n.n_reads, cl.thr, cl.n.n_segs, cl.spans);
}
