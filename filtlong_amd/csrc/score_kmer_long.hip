// score_kmer_long.hip — k-mer mode: the window fold of ultra-long reads and children, one WAVE per segment instead of one lane.
//
// A segment is a run of coverage bits: a read's whole row, or a child's range [start, end) of its parent's row.  The one-lane
// kernels (score_kmer.hip: k_kmer_fold) walk a segment serially, 32 positions per step; a 4 Mbp read is 131 072 dependent steps of
// one lane while the rest of the chip has long finished.  Here, for segments of at least a threshold of bases (score_kmer_common.h:
// FoldArgs::long_min — the batch kernels leave them alone):
//   1. k_kmer_long_words, chip-wide: for every step of 32 positions of every long segment the leading word (positions ws + 32 k ..)
//      and the trailing word (positions 32 k ..), funnel-shifted out of the row, and the summary of their +-1 walk — total, lowest
//      and highest prefix, from the nibble-pair table k_kmer_fold uses.  None of this depends on the window's value.
//   2. k_kmer_long_walk, one wave per segment: the head exactly as the one-lane kernel ((double)popcount(first ws bits) / ws), then
//      64 summaries at a time: a scan gives every word the regime's count in front of it, every lane tests its own word against the
//      regime's bounds, a ballot finds the first word that leaves the regime.  The words in front of it are applied in integers
//      (exact: fold_grid_tab.h), that word is replayed by the reference's own 32 floating-point steps, a regime begins on the value it
//      ends on, and the rest of the 64 summaries are tested again against the new bounds.  Only replays are serial.
//   3. with --trim / --split: k_kmer_long_children, one wave per long read, 64 words of the row at a time in integers — the zero
//      runs that start at 0, reach the end or are at least --split long, exactly MODE 3's / MODE 5's word-level events: once for
//      the count (before the offsets' scan), once to write child_ranges / child_parent in order (after it).  Children of at least the
//      threshold are segments of their own and go through 1. and 2.; the shorter ones stay with MODE 6.
// tools/sim_fold_long.cpp is the walk of 2. on the host against the plain recurrence, bit for bit.
#include "fold_common.h"

#include <cerrno>
#include <chrono>

namespace {

struct LongArgs {
    FoldArgs a;
    const uint32_t *ids;    // [n_seg] read index (reads) / child index (children) of every long segment
    const uint64_t *woff;   // [n_seg] its first word in sum / lw / tw
    uint32_t n_seg;
    int children;           // the segments are children
    uint32_t *sum;          // per word: total (int8) | lowest prefix (int8) << 8 | highest prefix << 16 | flags << 24
    uint32_t *lw, *tw;      // per word: the leading / the trailing 32 positions
    unsigned long long *replayed;  // words replayed in floating point (all segments of the call)
};
constexpr uint32_t kNonZero = 1u << 24;  // flags: one of the two words has a covered base
constexpr uint32_t kPartial = 2u << 24;  // the segment's last word, fewer than 32 positions: folded in floating point

struct Seg {
    const uint32_t *row;  // the coverage row the segment lies in
    int row_words;        // words of that row that hold coverage
    int start, len;       // the segment is bits [start, start + len) of the row
    uint32_t parent;      // the row's read
};

__device__ __forceinline__ Seg seg_of(const LongArgs &g, uint32_t id) {
    Seg s;
    if (!g.children) {
        s.parent = id;
        s.start = 0;
        s.len = g.a.lengths[id];
    } else {
        s.parent = g.a.child_parent[id];
        s.start = g.a.child_ranges[2 * (size_t)id];
        s.len = g.a.child_ranges[2 * (size_t)id + 1] - s.start;
    }
    s.row = g.a.cov + (g.a.cov_off[s.parent] >> 2);
    s.row_words = (g.a.lengths[s.parent] + 31) >> 5;
    return s;
}

// positions p .. p + 31 of the segment (p >= 0); positions behind its end read as uncovered
__device__ __forceinline__ uint32_t seg_bits32(const Seg &s, int p) {
    if (p >= s.len) return 0u;
    const int b = s.start + p, w = b >> 5;
    const uint32_t lo = w < s.row_words ? s.row[w] : 0u, hi = w + 1 < s.row_words ? s.row[w + 1] : 0u;
    uint32_t v = __builtin_amdgcn_alignbit(hi, lo, (unsigned)(b & 31));
    const int valid = s.len - p;
    if (valid < 32) v &= (1u << valid) - 1u;
    return v;
}

__device__ __forceinline__ int wave_sum(int v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ int wave_min(int v) {
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ int uniform_lane(int x, int lane) { return __shfl(x, lane, 64); }

// ---- the long reads of a batch, in no particular order: index and first word of each ----
__global__ void __launch_bounds__(256) k_kmer_long_find(uint64_t n, const int32_t *lengths, int thr, int ws, KmerLongCounts *cursor, uint32_t *ids,
                                                        uint64_t *woff) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int L = lengths[i];
    if (L < thr) return;
    const unsigned long long at = atomicAdd(&cursor->n, 1ull);
    ids[at] = (uint32_t)i;
    woff[at] = atomicAdd(&cursor->words, flx_kmer_long_words(L, ws));
}

// ---- 1. word summaries ----
__global__ void __launch_bounds__(256) k_kmer_long_words(const LongArgs g) {
    // the +-1 walk of four positions by (new nibble << 4 | old nibble), as in k_kmer_fold: total, lowest and highest prefix
    __shared__ uint32_t walk[256];
    {
        const int idx = threadIdx.x;
        int t = 0, mp = 0, xp = 0;
        for (int i = 0; i < 4; ++i) {
            t += ((idx >> (4 + i)) & 1) - ((idx >> i) & 1);
            mp = min(mp, t);
            xp = max(xp, t);
        }
        walk[idx] = ((uint32_t)t & 0xffu) | (((uint32_t)mp & 0xffu) << 8) | ((uint32_t)xp << 16);
    }
    __syncthreads();
    const int ws = g.a.ws;
    for (uint32_t si = blockIdx.y; si < g.n_seg; si += gridDim.y) {
        const Seg s = seg_of(g, g.ids[si]);
        const int nw = (int)flx_kmer_long_words(s.len, ws);
        const uint64_t at = g.woff[si];
        for (int k = (int)(blockIdx.x * 256u + threadIdx.x); k < nw; k += (int)(gridDim.x * 256u)) {
            const int valid = s.len - ws - 32 * k;  // positions of this step (>= 1)
            const uint32_t lead = seg_bits32(s, ws + 32 * k);
            uint32_t trail = seg_bits32(s, 32 * k);
            if (valid < 32) trail &= (1u << valid) - 1u;
            int run = 0, lo = 0, hi = 0;
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const uint32_t e = walk[(((lead >> (4 * q)) & 15u) << 4) | ((trail >> (4 * q)) & 15u)];
                lo = min(lo, run + (int)(int8_t)(e >> 8));
                hi = max(hi, run + (int)(e >> 16));
                run += (int)(int8_t)e;
            }
            uint32_t v = ((uint32_t)run & 0xffu) | (((uint32_t)lo & 0xffu) << 8) | ((uint32_t)hi << 16);
            if (lead | trail) v |= kNonZero;
            if (valid < 32) v |= kPartial;
            g.sum[at + k] = v;
            g.lw[at + k] = lead;
            g.tw[at + k] = trail;
        }
    }
}

// ---- 2. the walk ----
__global__ void __launch_bounds__(64) k_kmer_long_walk(const LongArgs g) {
    __shared__ double sh_ds[GridTab::kMax], sh_lv[GridTab::kMax];
    __shared__ int sh_top[GridTab::kMax];
    const int lane = threadIdx.x;
    if (lane < GridTab::kMax) {
        sh_ds[lane] = g.a.gt.dstar[lane];
        sh_lv[lane] = g.a.gt.lv[lane];
        sh_top[lane] = g.a.gt.top[lane];
    }
    __syncthreads();
    const uint32_t id = g.ids[blockIdx.x];
    const Seg s = seg_of(g, id);
    const int ws = g.a.ws, len = s.len;
    const double delta = g.a.delta;

    // the head: covered bases of the first window (of the whole segment, if it is no longer than the window)
    const int head = min(ws, len);
    int c0 = 0;
    for (int p = lane * 32; p < head; p += 64 * 32) {
        uint32_t v = seg_bits32(s, p);
        if (head - p < 32) v &= (1u << (head - p)) - 1u;
        c0 += __popc(v);
    }
    c0 = wave_sum(c0);
    int cnt = c0;  // covered bases of the segment (children: counted here; reads: the cover kernel's count)
    double w = 0.0, mn = 0.0;
    unsigned long long replays = 0;
    if (len > ws) {
        w = (double)c0 / g.a.ws_d;  // src/read.cpp:221-226
        mn = w;
        // the regime (all wave-uniform): w = r.wb + c * r.ds while r.lo <= c <= r.hi; lmin = lowest c this LANE's words reached
        GridRegime r;
        int c = 0, lmin = 0x7fffffff;
        auto begin = [&]() {  // fold_grid_tab.h: the table's entry of w's binade from LDS
            const int idx = grid_binade(w) - g.a.gt.e0;
            const bool has = w > 0.0 && idx >= 0 && idx < g.a.gt.n;
            r = grid_regime_begin(w, has ? sh_ds[idx] : 0.0, has ? sh_lv[idx] : 0.0, has ? sh_top[idx] : 0, g.a.ws_d);
            c = 0;
            lmin = 0x7fffffff;
        };
        auto flush = [&]() {  // the regime's state as the recurrence's: exact
            const int cmin = wave_min(lmin);
            if (cmin != 0x7fffffff) mn = fmin(mn, grid_value(r, cmin));
            w = grid_value(r, c);
        };
        begin();
        const int nw = (int)flx_kmer_long_words(len, ws);
        const uint32_t *sum = g.sum + g.woff[blockIdx.x], *lws = g.lw + g.woff[blockIdx.x], *tws = g.tw + g.woff[blockIdx.x];
        uint32_t n_sum = lane < nw ? sum[lane] : 0u, n_lw = lane < nw ? lws[lane] : 0u, n_tw = lane < nw ? tws[lane] : 0u;
        for (int k0 = 0; k0 < nw; k0 += 64) {
            const uint32_t sv = n_sum, lead = n_lw, trail = n_tw;
            {  // the next 64 words, a round ahead
                const int k = k0 + 64 + lane;
                n_sum = k < nw ? sum[k] : 0u;
                n_lw = k < nw ? lws[k] : 0u;
                n_tw = k < nw ? tws[k] : 0u;
            }
            if (g.children) cnt += __popc(lead);
            if (__ballot((sv & kNonZero) != 0u) == 0ull) continue;  // 64 words without a covered base on either edge: nothing moves
            const int t = (int)(int8_t)sv, mp = (int)(int8_t)(sv >> 8), xp = (int)((sv >> 16) & 0xffu);
            int incl = t;  // the regime's count behind this word, relative to the count in front of the 64
            for (int o = 1; o < 64; o <<= 1) {
                const int up = __shfl_up(incl, o, 64);
                if (lane >= o) incl += up;
            }
            const int pre = incl - t;
            int from = 0, pre_from = 0;
            for (;;) {
                const int ci = c + (pre - pre_from);
                const bool ok = !(sv & kNonZero) || (!(sv & kPartial) && ci + mp >= r.lo && ci + xp <= r.hi);
                const unsigned long long failed = __ballot(lane >= from && !ok);
                const int fail = failed ? __ffsll(failed) - 1 : 64;
                if (lane >= from && lane < fail) lmin = min(lmin, ci + mp);
                if (fail == 64) {
                    c += uniform_lane(incl, 63) - pre_from;
                    break;
                }
                c += uniform_lane(pre, fail) - pre_from;
                flush();
                // that word by the reference's own steps
                const uint32_t rl = (uint32_t)uniform_lane((int)lead, fail), rt = (uint32_t)uniform_lane((int)trail, fail);
                fold_word_fp<true>(w, mn, rl, rt, delta);
                ++replays;
                begin();
                pre_from = uniform_lane(incl, fail);
                from = fail + 1;
                if (from == 64) break;
            }
        }
        flush();
        if (g.children) cnt = c0 + wave_sum(cnt - c0);
    }
    if (lane != 0) return;
    if (replays) atomicAdd(g.replayed, replays);
    if (g.children) {
        const double mean = 100.0 * (double)cnt / (double)len;
        const double window = window_result(g.a, len, cnt, mn);
        g.a.child_mean_q[id] = mean;
        g.a.child_window_q[id] = window;
        g.a.child_passed[id] = cutoffs(g.a.p, len, mean, window);
    } else {
        cnt = g.a.count[id];
        const double mean = 100.0 * (double)cnt / (double)len;  // exact: the qualities are 0.0 / 1.0
        const double window = window_result(g.a, len, cnt, mn);
        g.a.mean_q[id] = mean;
        g.a.window_q[id] = window;
        g.a.passed[id] = cutoffs(g.a.p, len, mean, window);
    }
}

// ---- 3. bad ranges -> children of a long read (src/read.cpp:89-130; k_kmer_fold MODE 3 / MODE 5) ----
// Only a zero run that starts at position 0, reaches the end of the read or is at least --split (>= 32) long can be a bad range, and
// every run that ends is ended by the first covered base of a word that has one.  So per word with a covered base: the run in front
// of it began behind the last covered base of the nearest such word to the left (or at 0), and each lane decides on its own whether
// that run is bad; a ballot orders the bad ones, and the child in front of each reaches from the previous bad run's end to this one's
// start.  !EMIT: n_child of the read and how many of its children are long (totals); EMIT: child_ranges / child_parent in order,
// and the long children's places in the list (cursor).
template <bool EMIT>
__global__ void __launch_bounds__(64) k_kmer_long_children(const LongArgs g, KmerLongCounts *cc, uint32_t *c_ids, uint64_t *c_woff) {
    const int lane = threadIdx.x;
    const uint32_t rid = g.ids[blockIdx.x];
    const int L = g.a.lengths[rid];
    const uint32_t *row = g.a.cov + (g.a.cov_off[rid] >> 2);
    const int nw = (L + 31) >> 5;
    const ZeroRunRule rule(g.a.p);
    const int thr = g.a.long_min, ws = g.a.ws;
    const uint64_t cbase = EMIT ? g.a.child_offsets[rid] : 0;
    const unsigned long long below = (1ull << lane) - 1ull;
    // wave-uniform: one past the last covered base so far (0: none yet), start of the current child candidate, children so far
    int prev_tp = 0, cs = 0;
    bool any_bad = false;
    uint32_t nchild = 0;
    unsigned long long my_long = 0, my_words = 0;
    auto child = [&](uint32_t k, int start, int end) {  // child k of the read (one lane)
        const int len = end - start;
        if (EMIT) {
            const uint64_t at = cbase + k;
            g.a.child_ranges[2 * at] = start;
            g.a.child_ranges[2 * at + 1] = end;
            g.a.child_parent[at] = rid;
            if (len >= thr) {
                const unsigned long long slot = atomicAdd(&cc->n, 1ull);
                c_ids[slot] = (uint32_t)at;
                c_woff[slot] = atomicAdd(&cc->words, flx_kmer_long_words(len, ws));
            }
        } else if (len >= thr) {
            ++my_long;
            my_words += flx_kmer_long_words(len, ws);
        }
    };
    uint32_t nxt = lane < nw ? row[lane] : 0u;
    for (int k0 = 0; k0 < nw; k0 += 64) {
        const int k = k0 + lane, j0 = k * 32;
        uint32_t wd = nxt;
        nxt = k + 64 < nw ? row[k + 64] : 0u;
        if (k < nw && L - j0 < 32) wd &= (1u << (L - j0)) - 1u;
        const unsigned long long nzm = __ballot(wd != 0u);
        if (!nzm) continue;
        const int f = j0 + __ffs((int)wd) - 1;  // first covered base of the word
        const int tp = j0 + 32 - __clz((int)wd);  // one past its last one
        const unsigned long long nz_below = nzm & below;
        const int p = nz_below ? 63 - __clzll((long long)nz_below) : -1;
        const int tp_left = __shfl(tp, p < 0 ? 0 : p, 64);
        const int zs = p >= 0 ? tp_left : prev_tp;  // the zero run [zs, f) ends at this word's first covered base
        const bool bad = wd != 0u && f > zs && rule.bad_run(zs, f);
        const unsigned long long badm = __ballot(bad);
        if (badm) {
            const unsigned long long bad_below = badm & below;
            const int q = bad_below ? 63 - __clzll((long long)bad_below) : -1;
            const int f_left = __shfl(f, q < 0 ? 0 : q, 64);
            const int from = q >= 0 ? f_left : cs;  // the child in front of this bad range: [from, zs)
            const bool em = bad && zs > from;
            const unsigned long long emm = __ballot(em);
            if (em) child(nchild + (uint32_t)__popcll(emm & below), from, zs);
            nchild += (uint32_t)__popcll(emm);
            any_bad = true;
            cs = __shfl(f, 63 - __clzll((long long)badm), 64);
        }
        prev_tp = __shfl(tp, 63 - __clzll((long long)nzm), 64);
    }
    int end = L;
    if (prev_tp < L && rule.bad_run_at_end(prev_tp, L)) {  // the read ends inside the bad zero run [prev_tp, L)
        any_bad = true;
        end = prev_tp;
    }
    if (any_bad && end > cs) {
        if (lane == 0) child(nchild, cs, end);
        ++nchild;
    }
    if (!EMIT) {
        for (int o = 32; o > 0; o >>= 1) {
            my_long += __shfl_xor(my_long, o, 64);
            my_words += __shfl_xor(my_words, o, 64);
        }
        if (lane == 0) {
            g.a.n_child[rid] = nchild;
            if (my_long) {
                atomicAdd(&cc->n, my_long);
                atomicAdd(&cc->words, my_words);
            }
        }
    }
}

size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }

struct Layout {  // one list of long segments and their words inside a workspace
    size_t cursor, ids, woff, sum, lw, tw, end;
    explicit Layout(const KmerLongCounts &c) {
        size_t off = 0;
        cursor = off; off = up256(off + 64);  // KmerLongCounts cursor | words replayed (at + 32)
        ids = off; off = up256(off + c.n * 4);
        woff = off; off = up256(off + c.n * 8);
        sum = off; off = up256(off + c.words * 4);
        lw = off; off = up256(off + c.words * 4);
        tw = off; off = up256(off + c.words * 4);
        end = off;
    }
};

void long_args(LongArgs &g, const FoldArgs &a, const KmerLongCounts &c, char *base, bool children) {
    const Layout lay(c);
    g.a = a;
    g.ids = (const uint32_t *)(base + lay.ids);
    g.woff = (const uint64_t *)(base + lay.woff);
    g.n_seg = (uint32_t)c.n;
    g.children = children ? 1 : 0;
    g.sum = (uint32_t *)(base + lay.sum);
    g.lw = (uint32_t *)(base + lay.lw);
    g.tw = (uint32_t *)(base + lay.tw);
    g.replayed = (unsigned long long *)(base + lay.cursor + 32);
}

// summaries of every word of the list's segments, then one wave per segment
int launch_words_and_walk(flx_ctx *ctx, const LongArgs &g, const KmerLongCounts &c) {
    if (c.words > 0) {
        const uint64_t per_seg = (c.words + c.n - 1) / c.n;
        const unsigned gx = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(1024, (per_seg + 255) / 256));
        const unsigned gy = (unsigned)std::min<uint64_t>(c.n, 65535);
        hipLaunchKernelGGL(k_kmer_long_words, dim3(gx, gy), dim3(256), 0, ctx->stream, g);
    }
    hipLaunchKernelGGL(k_kmer_long_walk, dim3(g.n_seg), dim3(64), 0, ctx->stream, g);
    FLX_HIP(ctx, hipGetLastError());
    return FLX_OK;
}

double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

}  // namespace

// ---------------------------------------------------------------------------------------------------- host side
// Threshold: as in Phred mode (score_phred_long.hip) — the floor, doubled while the batch's bases per lane of the one-lane kernels
// are at least twice as many: a read no longer than a lane's share of the batch finishes inside the batch's time anyway.
// FLX_KMER_LONG_MIN: "0" = off, N = every read and child of at least N bases takes the path (tests).
#ifndef FLX_KMER_LONG_FLOOR
#define FLX_KMER_LONG_FLOOR (1 << 18)
#endif
int flx_kmer_long_threshold(flx_ctx *ctx, uint64_t plane_bytes, bool applies, KmerLong *kl) {
    *kl = KmerLong();
    long long thr = FLX_KMER_LONG_FLOOR;
    bool forced = false;
    const char *env = getenv("FLX_KMER_LONG_MIN");
    if (env) {
        char *end = nullptr;
        errno = 0;
        const unsigned long long v = strtoull(env, &end, 10);
        if (!*env || *end || errno || env[0] == '-' || env[0] == '+' || env[0] == ' ')
            return flx_fail(ctx, FLX_ERR_INVALID, "FLX_KMER_LONG_MIN=%s: expected a non-negative integer (bases)", env);
        if (v == 0 || v > 0x7fffffffull) return FLX_OK;  // off (no read is that long)
        thr = (long long)v;
        forced = true;
    }
    if (!applies) return FLX_OK;
    if (!forced) {
        const double per_lane = (double)plane_bytes / ((double)ctx->prop.multiProcessorCount * 1024.0);
        while (thr < (1ll << 30) && (double)(thr * 2) <= per_lane) thr *= 2;
    }
    kl->on = true;
    kl->thr = (int)thr;
    return FLX_OK;
}

size_t flx_kmer_long_reads_workspace(const KmerLongCounts &reads) { return Layout(reads).end; }
size_t flx_kmer_long_children_workspace(const KmerLongCounts &children) { return Layout(children).end; }

int flx_kmer_long_reads(flx_ctx *ctx, const FoldArgs &a, KmerLong *kl, const KmerLongCounts &reads, bool children, void *work, size_t work_bytes) {
    if (reads.n >= 0xffffffffull || work_bytes < Layout(reads).end) return flx_fail(ctx, FLX_ERR_INVALID, "k-mer long reads: workspace");
    LongArgs g;
    long_args(g, a, reads, (char *)work, false);
    hipStream_t st = ctx->stream;
    kl->n_reads_long = reads.n;
    kl->words += reads.words;
    kl->t_start = now_s();
    flx_time_scope ts(ctx, "flx_score_kmer_long");
    FLX_HIP(ctx, hipMemsetAsync(work, 0, 64, st));
    hipLaunchKernelGGL(k_kmer_long_find, dim3((unsigned)((a.n_reads + 255) / 256)), dim3(256), 0, st, a.n_reads, a.lengths, kl->thr, a.ws,
                       (KmerLongCounts *)work, (uint32_t *)g.ids, (uint64_t *)g.woff);
    FLX_CHECK(launch_words_and_walk(ctx, g, reads));
    if (children) hipLaunchKernelGGL((k_kmer_long_children<false>), dim3(g.n_seg), dim3(64), 0, st, g, kl->d_children, (uint32_t *)nullptr, (uint64_t *)nullptr);
    FLX_HIP(ctx, hipGetLastError());
    return FLX_OK;
}

int flx_kmer_long_children(flx_ctx *ctx, const FoldArgs &a, KmerLong *kl, const KmerLongCounts &reads, const KmerLongCounts &children, void *reads_work,
                           void *work, size_t work_bytes) {
    if (children.n >= 0xffffffffull || work_bytes < Layout(children).end) return flx_fail(ctx, FLX_ERR_INVALID, "k-mer long children: workspace");
    LongArgs gr, gc;
    long_args(gr, a, reads, (char *)reads_work, false);
    long_args(gc, a, children, (char *)work, true);
    hipStream_t st = ctx->stream;
    kl->n_children_long = children.n;
    kl->words += children.words;
    flx_time_scope ts(ctx, "flx_score_kmer_long");
    FLX_HIP(ctx, hipMemsetAsync(work, 0, 64, st));
    hipLaunchKernelGGL((k_kmer_long_children<true>), dim3(gr.n_seg), dim3(64), 0, st, gr, (KmerLongCounts *)work, (uint32_t *)gc.ids, (uint64_t *)gc.woff);
    if (children.n > 0) FLX_CHECK(launch_words_and_walk(ctx, gc, children));
    FLX_HIP(ctx, hipGetLastError());
    return FLX_OK;
}

int flx_kmer_long_report(flx_ctx *ctx, const KmerLong &kl, const void *reads_work, const void *children_work) {
    if (!getenv("FLX_API_TIMING") || kl.n_reads_long == 0) return FLX_OK;
    unsigned long long r0 = 0, r1 = 0;
    FLX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (reads_work) FLX_HIP(ctx, hipMemcpy(&r0, (const char *)reads_work + 32, 8, hipMemcpyDeviceToHost));
    if (children_work) FLX_HIP(ctx, hipMemcpy(&r1, (const char *)children_work + 32, 8, hipMemcpyDeviceToHost));
    fprintf(stderr, "[flx_score_batch] %-22s %8.3f ms  (%llu reads and %llu children of >= %d bases, %llu words, %llu replayed)\n", "kmer long reads",
            (now_s() - kl.t_start) * 1e3, (unsigned long long)kl.n_reads_long, (unsigned long long)kl.n_children_long, kl.thr,
            (unsigned long long)kl.words, r0 + r1);
    return FLX_OK;
}
