// score_kmer.hip — k-mer mode per-read scoring on gfx950: the window folds over the coverage bits, and the call that runs both stages.
//
// Replaces the k-mer branch of the reference's Read::Read: first/last covered base (src/read.cpp:75-84), bad ranges /
// trim / split -> child ranges (86-130) and the scoring of every child read (131-141), plus the shared
// mean / window / cut-off code (208-236, 64-73).  The lookups that turn the seq plane into the coverage bit plane (43-58) are the
// coverage stage's: cover_common.h (flx_kmer_cover_stage), cover_wave.hip, cover_queue.hip, cover_long.hip.
//
//   k_kmer_fold   (read-serial)  one lane per read walks its coverage bits and replays get_window_quality
//                 bit-exactly (w -= q[i]/ws; w += q[j]/ws with q/ws in {0, fl(1/ws)}: the drift is real,
//                 SURVEY §8c test_trim_3 = 0x1.5ffffffffffffp+6), and — under --trim/--split — finds the bad
//                 zero-runs, the child ranges, and runs the same recurrence for every child on the fly.
//                 Children never have grandchildren (their coverage is a slice of the parent's),
//                 so a child's mean/window/cut-offs come from the parent's bits without new lookups.
#include "flx_internal.h"
#include "kmerset.h"
#include "cover_common.h"
#include "rank_internal.h"
#include "fold_common.h"

namespace {

// ---------------------------------------------------------------------------------------------------
// serial fold over the coverage bits
// ---------------------------------------------------------------------------------------------------
// (the modes, the row as a lane sees it, the zero-run rule and the steps of one word: fold_common.h; the grid table and the start of
// a regime: fold_grid_tab.h; the folds' arguments and the shared result code: score_kmer_common.h)
// One lane per slot — a read, or in the mode whose slots are children a child — and per word of 32 positions four phases:
// the zero-run events of the word, the head shortcut, the steady state, the positions one by one.  What a mode does in each is
// kFoldModes' to say.  The register budget was A/B-built with amdgpu_waves_per_eu and left to the compiler: no setting won.
template <int MODE, bool RING, bool GRID = false>
__global__ void __launch_bounds__(256) k_kmer_fold(const FoldArgs a) {
    constexpr FoldMode M = kFoldModes[MODE];
    constexpr bool kChild = M.child;
    const uint64_t slot = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool live = slot < (kChild ? a.n_children : a.n_reads);
    uint32_t rid = 0;  // the read's index, or the child's
    int L = 0;
    FoldRow row;
    row.row = a.cov;
    row.bit_off = 0;
    int row_words_left = 0;  // a child: words of the parent's row from row.row on
    if (live && !kChild) {
        rid = a.order ? a.order[slot] : (uint32_t)slot;
        L = a.lengths[rid];
        row.row = a.cov + (a.cov_off[rid] >> 2);
    }
    if (live && kChild) {
        rid = a.child_order[slot];
        const uint32_t parent = a.child_parent[rid];
        const int start = a.child_ranges[2 * (size_t)rid], end = a.child_ranges[2 * (size_t)rid + 1];
        L = end - start;
        const int base_word = (start >> 7) << 2;  // 16-byte aligned piece of the row the child starts in
        row.row = a.cov + (a.cov_off[parent] >> 2) + base_word;
        row_words_left = ((a.lengths[parent] + 31) >> 5) - base_word;
        row.bit_off = (uint32_t)(start - 32 * base_word);
    }
    if (M.leaves_long && a.long_min > 0 && L >= a.long_min) {
        // a long read or child: the cooperative path's (score_kmer_long.hip) — this lane folds nothing and writes nothing
        live = false;
        L = 0;
    }
    int Lmax = L;
    for (int o = 32; o > 0; o >>= 1) Lmax = max(Lmax, __shfl_xor(Lmax, o, 64));
    const int ws = a.ws;

    Win P = {0, 0.0, 0.0};
    Children K;
    const uint64_t cbase = ((M.out & kOutRanges) && live) ? a.child_offsets[rid] : 0;
    const ZeroRunRule rule(a.p);

    row.n_words = kChild ? row_words_left : (L + 31) >> 5;
    extern __shared__ uint32_t fold_lds[];  // GRID: the walk table and the grid table (kGridLdsWords dwords); then the rings
    if (GRID) grid_lds_fill(fold_lds, a.gt);
    row.R = a.ring_words;
    row.ring = fold_lds + (GRID ? kGridLdsWords : 0) + (size_t)(threadIdx.x >> 6) * (size_t)row.R * 64 + (threadIdx.x & 63);
    row.begin<RING>();
    int Lmin = live ? L : 0x7fffffff;
    for (int o = 32; o > 0; o >>= 1) Lmin = min(Lmin, __shfl_xor(Lmin, o, 64));
    GridLane g;
    uint32_t trail_w = 0;  // the trailing edge's word of the per-position phase
    for (int j0 = 0; j0 < Lmax; j0 += 32) {
        uint32_t lead_w = row.lead_word<RING, kChild>(j0 >> 5);
        // ---- 1. events: the zero runs that end or begin in this word ----
        if (M.events == kEvWord) {
            const ZeroRunWord z = zero_run_word(rule, lead_w, j0, L, K.zs);
            if (M.window == kWinChildWords) {  // the children's own recurrence, in this lane
                child_word_positions<RING, M.out>(a, row, j0, L, lead_w, z, K, rid, cbase);
                continue;
            }
            if (z.ev_end >= 0) {
                K.any_bad = true;
                emit_child<M.out>(a, rid, cbase, K.n, K.cs, z.ev_zs, K.S);  // (counts it, and writes what the mode writes)
                K.cs = j0 + z.ev_end;
            }
            if (M.window == kWinNone) continue;
        }
        // ---- 2. the head, a word at a time: every position of the word lies in front of the first full window (j < ws - 1) and inside
        // every read of the wave — the recurrence has not begun, only the covered bases are counted (src/read.cpp:221-225).  (The
        // per-position loop spent ~20 instructions on each of these positions: a fifth of a 10 kbp read's fold once the steady state
        // ran on the integer grid.)
        if (M.window == kWinWords && j0 + 32 <= ws - 1 && j0 + 32 <= Lmin) {
            P.cnt += __popc(lead_w);
            continue;
        }
        // ---- 3. steady state, one window per lane: the word's 32 positions at once (fold_word_*) ----
        if (M.window == kWinWords && j0 >= ws && j0 + 32 <= Lmin) {
            uint32_t tw = row.trail32<RING, kChild>(j0 - ws);
            P.cnt += __popc(lead_w);
            if (GRID) {
                fold_word_grid(g, P, lead_w, tw, fold_lds, a);
                continue;
            }
            if (a.events && fold_word_events(P, lead_w, tw, a.delta)) continue;
            fold_word_fp<false>(P.w, P.mn, lead_w, tw, a.delta);
            continue;
        }
        // ---- 4. per position (the shortest read of the wave ends inside this word, or the mode has no steady state) ----
        if (GRID && g.on) {  // the steady state is over: back to the recurrence's own state
            grid_flush(g, P);
            g.on = false;
            g.r.ds = 0.0;
            g.c = g.cmin = 0;
            g.r.wb = P.w;
        }
        fold_positions<RING, kChild, M.events, M.out>(a, row, j0, L, Lmax, lead_w, trail_w, P, rule, K, rid, cbase);
    }
    if (GRID && g.on) grid_flush(g, P);
    if (!live) return;

    if (M.out & kOutOwnScores) {  // the child's own scores (src/read.cpp:131-137 -> the Read constructor's folds on the child's slice)
        const double mean = 100.0 * (double)P.cnt / (double)L;
        const double window = window_result(a, L, P.cnt, P.mn);
        a.child_mean_q[rid] = mean;
        a.child_window_q[rid] = window;
        a.child_passed[rid] = cutoffs(a.p, L, mean, window);
        return;
    }
    if (M.events != kEvNone) {
        int end = L;
        if (K.zs >= 0 && rule.bad_run_at_end(K.zs, L)) {  // the read ends inside a bad zero run [zs, L)
            K.any_bad = true;
            end = K.zs;
            K.C = K.S;
        }
        if (K.any_bad) emit_child<M.out>(a, rid, cbase, K.n, K.cs, end, K.C);
        else K.n = 0;
    }
    if (M.out & kOutCount) a.n_child[rid] = K.n;
    if (M.out & kOutRead) {
        const double mean = 100.0 * (double)a.count[rid] / (double)L;  // exact: the qualities are 0.0 / 1.0
        const double window = window_result(a, L, P.cnt, P.mn);
        a.mean_q[rid] = mean;
        a.window_q[rid] = window;
        a.passed[rid] = cutoffs(a.p, L, mean, window);
    }
}

// (long_min > 0: also counts the batch's long reads and their 32-position steps for the cooperative path, score_kmer_long.hip;
// cover_min > 0: the reads the coverage stage covers in segments, and their segments — cover_long.hip)
__global__ void k_cov_row_bytes(uint64_t n, const int32_t *lengths, int64_t *row_bytes, int long_min, int ws, KmerLongCounts *long_reads,
                                int cover_min, int seg_bases, CoverLongCounts *cover_long) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int L = lengths[i];
    row_bytes[i] = (int64_t)((((uint64_t)L + 7) / 8 + 15) & ~15ull);
    if (long_min > 0 && L >= long_min) {
        atomicAdd(&long_reads->n, 1ull);
        atomicAdd(&long_reads->words, flx_kmer_long_words(L, ws));
    }
    if (cover_min > 0 && L >= cover_min) {
        atomicAdd(&cover_long->n_reads, 1ull);
        atomicAdd(&cover_long->n_segs, (unsigned long long)flx_cover_seg_count(L, seg_bases));
    }
}

__global__ void k_widen_u32_i64(uint64_t n, const uint32_t *in, int64_t *out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = (int64_t)in[i];
}

// the ranges MODE 3 left inline -> their places in the CSR (+ every child's read); counts the reads that have more than fit inline
__global__ void __launch_bounds__(256) k_children_from_inline(uint64_t n, const uint32_t *n_child, const uint64_t *child_offsets, const int32_t *inline_ranges,
                                                              int32_t *child_ranges, uint32_t *child_parent, unsigned int *overflow,
                                                              const int32_t *lengths, int long_min) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t nc = n_child[i];
    if (nc == 0) return;
    if (long_min > 0 && lengths[i] >= long_min) return;  // a long read: the cooperative path writes its ranges, however many
    if (nc > (uint32_t)kInlineChildren) {
        atomicAdd(overflow, 1u);
        return;
    }
    const uint64_t at = child_offsets[i];
    const int32_t *src = inline_ranges + (size_t)i * kInlineChildren * 2;
    for (uint32_t k = 0; k < nc; ++k) {
        child_ranges[2 * (at + k)] = src[2 * k];
        child_ranges[2 * (at + k) + 1] = src[2 * k + 1];
        child_parent[at + k] = (uint32_t)i;
    }
}

// sort key of a child: longest first (the lanes of a wave then run the same number of steps)
__global__ void k_child_keys(uint64_t n, const int32_t *ranges, uint64_t *keys, uint32_t *vals) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        keys[i] = (uint64_t)(0x7fffffffu - (uint32_t)(ranges[2 * i + 1] - ranges[2 * i]));
        vals[i] = (uint32_t)i;
    }
}

}  // namespace

// the fold kernels: with the LDS ring when it fits (R words per lane; 4 waves per workgroup up to R = 64, one wave up to R = 512),
// else (windows beyond ~15 000 positions) both streams from global memory
// The timing bracket of a fold launch says which form ran: flx_score_kmer_fold.m<MODE>.<ring<R> | global>.<fp | grid>.  Every name is
// a static string (the context keeps the pointer) and complete, so none is a prefix of another; flx_timing_get("flx_score_kmer_fold")
// still sums all of them — one bracket per launch, none nested, so that sum is the device time of the folds.
#define FLX_FOLD_NAMES_PATH(m, path) {"flx_score_kmer_fold.m" #m "." path ".fp", "flx_score_kmer_fold.m" #m "." path ".grid"}
#define FLX_FOLD_NAMES_MODE(m)                                                                                         \
    {FLX_FOLD_NAMES_PATH(m, "ring32"), FLX_FOLD_NAMES_PATH(m, "ring64"), FLX_FOLD_NAMES_PATH(m, "ring128"),            \
     FLX_FOLD_NAMES_PATH(m, "ring256"), FLX_FOLD_NAMES_PATH(m, "ring512"), FLX_FOLD_NAMES_PATH(m, "global")}
static const char *const kFoldTimingNames[7][6][2] = {FLX_FOLD_NAMES_MODE(0), FLX_FOLD_NAMES_MODE(1), FLX_FOLD_NAMES_MODE(2), FLX_FOLD_NAMES_MODE(3),
                                                      FLX_FOLD_NAMES_MODE(4), FLX_FOLD_NAMES_MODE(5), FLX_FOLD_NAMES_MODE(6)};
#undef FLX_FOLD_NAMES_MODE
#undef FLX_FOLD_NAMES_PATH

template <int MODE>
static int launch_fold(flx_ctx *ctx, FoldArgs &a) {
    int R = 32, path = 0;  // path: 0..4 = the ring of 32 << path words, 5 = global streams
    while (R < (MODE == 6 ? 24 : 18) + (a.ws + 31) / 32) R *= 2, ++path;  // MODE 6 starts up to 4 words into its first block, and reads one word further
    const char *env = getenv("FLX_KMER_FOLD_STREAMS");  // "global": the round-2 data path (second implementation, tests)
    const bool ring = R <= 512 && !(env && strcmp(env, "global") == 0);
    if (!ring) path = 5;
    const unsigned threads = (!ring || R <= 64) ? 256u : 64u;
    const unsigned nb = (unsigned)(((MODE == 6 ? a.n_children : a.n_reads) + threads - 1) / threads);
    a.ring_words = R;
    const bool grid = ring && a.grid && !a.events && (MODE == 0 || MODE == 3 || MODE == 6);  // the steady state on the integer grid (GridTab)
    if (grid) {
        constexpr int M = (MODE == 0 || MODE == 3 || MODE == 6) ? MODE : 0;
        ctx->last_kmer_fold_grid = true;
        const size_t lds = (size_t)(threads / 64) * (size_t)R * 256 + kGridLdsWords * 4;
        FLX_HIP(ctx, hipFuncSetAttribute((const void *)k_kmer_fold<M, true, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        flx_time_scope tf(ctx, kFoldTimingNames[MODE][path][1]);
        hipLaunchKernelGGL((k_kmer_fold<M, true, true>), dim3(nb), dim3(threads), lds, ctx->stream, a);
    } else if (ring) {
        const size_t lds = (size_t)(threads / 64) * (size_t)R * 256;
        FLX_HIP(ctx, hipFuncSetAttribute((const void *)k_kmer_fold<MODE, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        flx_time_scope tf(ctx, kFoldTimingNames[MODE][path][0]);
        hipLaunchKernelGGL((k_kmer_fold<MODE, true>), dim3(nb), dim3(threads), lds, ctx->stream, a);
    } else {
        flx_time_scope tf(ctx, kFoldTimingNames[MODE][path][0]);
        hipLaunchKernelGGL((k_kmer_fold<MODE, false>), dim3(nb), dim3(threads), 0, ctx->stream, a);
    }
    FLX_HIP(ctx, hipGetLastError());  // (a launch that fails must not pass for a kernel that wrote nothing)
    return FLX_OK;
}

// How a call folds, decided once from the parameters and the environment.  The switches select second implementations that the
// tests hold against the default ones; an unknown value of FLX_KMER_FOLD is a variant like the others (no inline ranges, no
// cooperative path) that then takes the default launches.
struct FoldPlan {
    bool bit_level;        // zero runs per bit (MODE 1 + 2): --split < 32, where a run inside one word can be a bad range, or FLX_KMER_FOLD=bits
    bool per_child;        // one lane per child (MODE 3, 5, 6); else FLX_KMER_FOLD=words: the children inside their read's lane (MODE 3 + 4)
    bool inline_children;  // MODE 3 leaves every read's first ranges beside it (FoldArgs::inline_ranges)
    bool grid;             // the steady state on the integer grid; FLX_KMER_FOLD_GRID=0 and windows whose table does not pay: in floating point
    bool events;           // FLX_KMER_FOLD_EVENTS=1
    // The cooperative path for ultra-long reads and children (score_kmer_long.hip) applies where the one-lane kernels would fold on
    // the integer grid: a window size whose grid table pays, none of the test-only fold variants, --split absent or >= 32.
    bool cooperative;
};
static FoldPlan fold_plan(const flx_params *params, bool want_children, bool grid_pays) {
    const char *fold_env = getenv("FLX_KMER_FOLD"), *ev_env = getenv("FLX_KMER_FOLD_EVENTS"), *grid_env = getenv("FLX_KMER_FOLD_GRID");
    const bool short_split = params->split_set && params->split < 32;
    FoldPlan p;
    p.bit_level = short_split || (fold_env && strcmp(fold_env, "bits") == 0);
    p.per_child = !p.bit_level && !(fold_env && strcmp(fold_env, "words") == 0);
    p.inline_children = want_children && !short_split && !fold_env;
    p.grid = grid_pays && !(grid_env && grid_env[0] == '0');
    p.events = ev_env && ev_env[0] == '1';
    p.cooperative = p.grid && !p.events && !fold_env && !short_split;
    return p;
}

int flx_score_kmer_dev(flx_ctx *ctx, const flx_kmerset *set, const uint8_t *d_plane, uint64_t plane_bytes,
                       const uint64_t *d_offsets, const int32_t *d_lengths, const uint32_t *d_order,
                       uint64_t n_reads, const flx_params *params, flx_scores *out) {
    out->n_children = 0;
    ctx->last_kmer_redo = nullptr;  // (they name workspace 0 of the previous call: not past the first return of this one)
    ctx->last_kmer_redo_n = 0;
    ctx->last_kmer_cover = "";
    if (n_reads == 0) return FLX_OK;
    hipStream_t st = ctx->stream;
    const bool want_children = params->trim || params->split_set;
    if (want_children && !out->child_offsets)
        return flx_fail(ctx, FLX_ERR_INVALID, "trim/split requested but child_offsets is NULL");
    const unsigned nb = (unsigned)((n_reads + 255) / 256);

    // ---- coverage plane layout: row i = ceil(L/8) bytes rounded up to 16, rows packed by an exclusive scan ----
    // All device memory of this path comes from the context's two grow-only workspaces: nothing is allocated or freed per
    // batch once they have reached their size.
    const size_t scan_ws = flx_radix_sort_workspace(n_reads + 1);
    auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
    GridTab gt;
    const FoldPlan plan = fold_plan(params, want_children, build_grid_table(params->window_size, gt));
    KmerLong kl;
    FLX_CHECK(flx_kmer_long_threshold(ctx, plane_bytes, plan.cooperative, &kl));
    // The cooperative path of the coverage stage (cover_long.hip): long reads are covered as segments, one wave each, by the
    // wave-level kernels — whatever the window size, --split and the fold variant; the workgroup-per-read form keeps them in its own launch
    CoverLong cvl;
    FLX_CHECK(flx_cover_long_threshold(ctx, plane_bytes, !flx_kmer_cover_is_v2(set), &cvl));
    const size_t small_bytes = 2 * up((n_reads + 1) * 8) + 3 * up(n_reads * 4) + up((n_reads + 1) * 4) + up(scan_ws) + up(n_reads) +
                               (plan.inline_children ? up(n_reads * (size_t)kInlineChildren * 8) + up(64) : 0) + up(64);
    void *small = nullptr;
    FLX_CHECK(flx_workspace(ctx, 0, small_bytes, &small));
    char *wp = (char *)small;
    auto carve = [&](size_t bytes) { void *q = wp; wp += up(bytes); return q; };
    int64_t *d_rowb = (int64_t *)carve((n_reads + 1) * 8);
    int64_t *d_covoff = (int64_t *)carve((n_reads + 1) * 8);
    int32_t *d_cnt = (int32_t *)carve(n_reads * 4);
    int32_t *d_first_tmp = (int32_t *)carve(n_reads * 4);
    int32_t *d_last_tmp = (int32_t *)carve(n_reads * 4);
    uint32_t *d_nchild = (uint32_t *)carve((n_reads + 1) * 4);
    void *d_scanws = carve(scan_ws);
    uint8_t *d_redo = (uint8_t *)carve(n_reads);  // cover_queue.hip: marks of the reads handed to the kernel with a diagonal per lane
    int32_t *d_inline = plan.inline_children ? (int32_t *)carve(n_reads * (size_t)kInlineChildren * 8) : nullptr;
    unsigned int *d_overflow = plan.inline_children ? (unsigned int *)carve(64) : nullptr;
    int32_t *first = out->first ? out->first : d_first_tmp, *last = out->last ? out->last : d_last_tmp;
    // the counters of the cooperative paths, 64 bytes: the long reads' and (at + 1) the long children's counts for the folds, then
    // the coverage stage's long reads and segments — zeroed by one memset, read back by one copy with the wait below
    struct LongCounters {
        KmerLongCounts reads, children;
        CoverLongCounts cover;
    };
    static_assert(sizeof(LongCounters) == 64, "the counters' block");
    LongCounters *d_counters = (LongCounters *)carve(64);
    kl.d_reads = &d_counters->reads;
    kl.d_children = &d_counters->children;
    FLX_HIP(ctx, hipMemsetAsync(d_rowb, 0, (n_reads + 1) * 8, st));
    if (kl.on || cvl.on) FLX_HIP(ctx, hipMemsetAsync(d_counters, 0, sizeof(LongCounters), st));
    hipLaunchKernelGGL(k_cov_row_bytes, dim3(nb), dim3(256), 0, st, n_reads, d_lengths, d_rowb, kl.on ? kl.thr : 0, params->window_size, kl.d_reads,
                       cvl.on ? cvl.thr : 0, cvl.spans * 1024, &d_counters->cover);
    FLX_CHECK(flx_exclusive_scan_i64(ctx, n_reads + 1, d_rowb, d_covoff, d_scanws, scan_ws));
    int64_t cov_bytes = 0;
    KmerLongCounts long_reads = {0, 0}, long_children = {0, 0};
    LongCounters counters;
    memset(&counters, 0, sizeof counters);
    FLX_HIP(ctx, hipMemcpyAsync(&cov_bytes, d_covoff + n_reads, 8, hipMemcpyDeviceToHost, st));
    if (kl.on || cvl.on) FLX_HIP(ctx, hipMemcpyAsync(&counters, d_counters, sizeof counters, hipMemcpyDeviceToHost, st));  // (with the wait below)
    FLX_HIP(ctx, hipStreamSynchronize(st));
    long_reads = counters.reads;
    cvl.n = counters.cover;
    void *d_cov = nullptr;
    const size_t cov_room = up((size_t)cov_bytes + 64), long_room = long_reads.n ? flx_kmer_long_reads_workspace(long_reads) : 0;
    const size_t cover_long_room = cvl.n.n_segs ? flx_cover_long_workspace(cvl.n) : 0;
    const size_t cover_long_at = up(cov_room + long_room);
    FLX_CHECK(flx_workspace(ctx, 1, cover_long_at + cover_long_room, &d_cov));
    void *d_long_reads = long_reads.n ? (char *)d_cov + cov_room : nullptr, *d_long_children = nullptr;
    void *d_cover_long = cvl.n.n_segs ? (char *)d_cov + cover_long_at : nullptr;

    // ---- stage 1: lookups -> coverage bits (cover_common.h) ----
    FLX_CHECK(flx_kmer_cover_stage(ctx, set, d_plane, d_offsets, d_lengths, d_order, n_reads, (uint32_t *)d_cov, (const uint64_t *)d_covoff, d_cnt, first, last,
                                   d_redo, cvl, &d_counters->cover, d_cover_long, cover_long_room));

    // ---- stage 2: serial fold ----
    FoldArgs a;  // (what a launch does not use stays null / 0: the struct's defaults)
    a.cov = (uint32_t *)d_cov;
    a.cov_off = (const uint64_t *)d_covoff;
    a.lengths = d_lengths;
    a.order = d_order;
    a.n_reads = n_reads;
    a.count = d_cnt;
    a.first = first;
    a.last = last;
    a.ws = params->window_size;
    a.ws_d = (double)(size_t)params->window_size;
    {
        volatile double one = 1.0, half = 0.5, wsd = a.ws_d;
        a.delta = one / wsd;
        a.clamp = half / wsd;
    }
    a.p = *params;
    a.gt = gt;
    a.events = plan.events;
    a.grid = plan.grid;
    a.long_min = kl.on ? kl.thr : 0;
    ctx->last_kmer_fold_grid = false;  // (launch_fold says so when a grid kernel really runs)
    a.mean_q = out->mean_q;
    a.window_q = out->window_q;
    a.passed = out->passed;
    a.inline_ranges = d_inline;
    a.child_ranges = out->child_ranges;
    a.child_mean_q = out->child_mean_q;
    a.child_window_q = out->child_window_q;
    a.child_passed = out->child_passed;

    // (every fold launch opens its own timing bracket: launch_fold)
    if (!want_children) {
        FLX_CHECK(launch_fold<0>(ctx, a));
        if (long_reads.n) FLX_CHECK(flx_kmer_long_reads(ctx, a, &kl, long_reads, false, d_long_reads, long_room));
        if (out->child_offsets) FLX_HIP(ctx, hipMemsetAsync(out->child_offsets, 0, (n_reads + 1) * 8, st));
        FLX_HIP(ctx, hipGetLastError());
        FLX_HIP(ctx, hipStreamSynchronize(st));
        flx_cover_long_report(cvl);
        return flx_kmer_long_report(ctx, kl, d_long_reads, nullptr);
    }

    FLX_HIP(ctx, hipMemsetAsync(d_nchild, 0, (n_reads + 1) * 4, st));
    a.n_child = d_nchild;
    if (plan.bit_level)
        FLX_CHECK(launch_fold<1>(ctx, a));  // runs inside one word can be bad ranges
    else
        FLX_CHECK(launch_fold<3>(ctx, a));
    // the long reads: their folds, their n_child, and how many of their children are long themselves
    if (long_reads.n) FLX_CHECK(flx_kmer_long_reads(ctx, a, &kl, long_reads, true, d_long_reads, long_room));
    // child_offsets = exclusive scan of the counts (n + 1 entries; the last one is the total)
    hipLaunchKernelGGL(k_widen_u32_i64, dim3((unsigned)((n_reads + 1 + 255) / 256)), dim3(256), 0, st, n_reads + 1,
                       d_nchild, d_rowb);
    FLX_CHECK(flx_exclusive_scan_i64(ctx, n_reads + 1, d_rowb, (int64_t *)out->child_offsets, d_scanws, scan_ws));
    int64_t total_children = 0;
    FLX_HIP(ctx, hipMemcpyAsync(&total_children, (int64_t *)out->child_offsets + n_reads, 8, hipMemcpyDeviceToHost, st));
    if (long_reads.n) FLX_HIP(ctx, hipMemcpyAsync(&long_children, kl.d_children, sizeof long_children, hipMemcpyDeviceToHost, st));
    FLX_HIP(ctx, hipStreamSynchronize(st));
    out->n_children = (uint64_t)total_children;
    if ((uint64_t)total_children > out->child_capacity)
        return flx_fail(ctx, FLX_ERR_CAPACITY, "child outputs need room for %lld children (capacity %llu)",
                        (long long)total_children, (unsigned long long)out->child_capacity);
    if (total_children > 0) {
        a.child_offsets = out->child_offsets;
        if (plan.bit_level) {
            FLX_CHECK(launch_fold<2>(ctx, a));
        } else if (!plan.per_child) {
            FLX_CHECK(launch_fold<4>(ctx, a));
        } else {
            // ranges (word-level events only) -> children by descending length -> one lane per child
            const uint64_t nc = (uint64_t)total_children;
            const size_t sort_ws = flx_radix_sort_workspace(nc);
            void *cw = nullptr;
            const size_t long_child_room = long_reads.n ? flx_kmer_long_children_workspace(long_children) : 0;
            FLX_CHECK(flx_workspace(ctx, 2, 2 * up(nc * 8) + 3 * up(nc * 4) + up(sort_ws) + long_child_room, &cw));
            wp = (char *)cw;
            uint64_t *keys0 = (uint64_t *)carve(nc * 8), *keys1 = (uint64_t *)carve(nc * 8);
            uint32_t *vals0 = (uint32_t *)carve(nc * 4), *vals1 = (uint32_t *)carve(nc * 4);
            a.child_parent = (uint32_t *)carve(nc * 4);
            void *d_sortws = carve(sort_ws);
            if (long_reads.n) d_long_children = carve(long_child_room);
            a.n_children = nc;
            unsigned int overflow = 1;
            if (d_inline) {  // the ranges MODE 3 left inline go to their places; a read with more than fit sends the batch through MODE 5
                FLX_HIP(ctx, hipMemsetAsync(d_overflow, 0, 4, st));
                {
                    flx_time_scope ti(ctx, "flx_score_kmer_fold.inline");  // (part of the folds' device time; closed before the host waits)
                    hipLaunchKernelGGL(k_children_from_inline, dim3(nb), dim3(256), 0, st, n_reads, (const uint32_t *)d_nchild, (const uint64_t *)out->child_offsets,
                                       (const int32_t *)d_inline, out->child_ranges, a.child_parent, d_overflow, d_lengths, a.long_min);
                }
                FLX_HIP(ctx, hipMemcpyAsync(&overflow, d_overflow, 4, hipMemcpyDeviceToHost, st));
                FLX_HIP(ctx, hipStreamSynchronize(st));
            }
            if (overflow) FLX_CHECK(launch_fold<5>(ctx, a));
            // the long reads' ranges, and the folds of the children that are long themselves (MODE 6 below leaves those alone)
            if (long_reads.n) FLX_CHECK(flx_kmer_long_children(ctx, a, &kl, long_reads, long_children, d_long_reads, d_long_children, long_child_room));
            hipLaunchKernelGGL(k_child_keys, dim3((unsigned)((nc + 255) / 256)), dim3(256), 0, st, nc, out->child_ranges, keys0, vals0);
            uint64_t *skeys = nullptr;
            uint32_t *svals = nullptr;
            FLX_CHECK(flx_radix_sort_pairs(ctx, nc, keys0, keys1, vals0, vals1, d_sortws, sort_ws, &skeys, &svals));
            a.child_order = svals;
            FLX_CHECK(launch_fold<6>(ctx, a));
        }
    }
    FLX_HIP(ctx, hipGetLastError());
    FLX_HIP(ctx, hipStreamSynchronize(st));
    flx_cover_long_report(cvl);
    return flx_kmer_long_report(ctx, kl, d_long_reads, d_long_children);
}
