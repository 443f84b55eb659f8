// score_kmer_common.h — what the k-mer fold kernels of score_kmer.hip (one lane per read or child) and score_kmer_long.hip (one
// wave per long read or child) share: the folds' arguments, the result code, and the protocol between the two.
#pragma once

#include "flx_internal.h"
#include "fold_grid_tab.h"

constexpr int kInlineChildren = 8;
struct FoldArgs {
    GridTab gt;
    const uint32_t *cov;
    const uint64_t *cov_off;
    const int32_t *lengths;
    const uint32_t *order;
    uint64_t n_reads;
    const int32_t *count;
    const int32_t *first;
    const int32_t *last;
    int ws;
    int ring_words;  // RING kernels: words per lane in the LDS ring (a power of two)
    int events;      // FLX_KMER_FOLD_EVENTS=1: the steady state walks the positions where the window's edges differ (measured: not faster)
    int grid;        // 1: the steady state runs on the integer grid (GridTab below; FLX_KMER_FOLD_GRID=0 and windows without a wide group: 0)
    // Reads and children of at least long_min bases (0: none) belong to the cooperative path (score_kmer_long.hip): their lane in
    // MODE 0 / 3 / 5 / 6 is not live — it folds nothing and writes nothing
    int long_min;
    double ws_d;
    double delta;  // fl(1.0 / ws): the value of q/ws for a covered base (src/read.cpp:228-229)
    double clamp;  // 0.5 / ws
    flx_params p;
    double *mean_q;
    double *window_q;
    uint8_t *passed;
    // MODE 3 leaves the first kInlineChildren ranges of every read here ([n_reads][kInlineChildren][2], or NULL): they are moved to
    // their places in the CSR once the counts have been scanned, and the ranges pass (MODE 5) only runs for a batch in which some
    // read has more (round 5: MODE 5 walked every row again for ~1 child per read — 7.7 of C4's 33 ms of folds)
    int32_t *inline_ranges = nullptr;
    // MODE 5 / 6: one lane per child
    uint32_t *child_parent = nullptr;         // [n_children] read index of every child (written by MODE 5, read by MODE 6)
    const uint32_t *child_order = nullptr;    // [n_children] children by descending length (MODE 6)
    uint64_t n_children = 0;
    // children
    uint32_t *n_child = nullptr;              // [n] (count pass)
    const uint64_t *child_offsets = nullptr;  // [n+1] (emit pass)
    int32_t *child_ranges;
    double *child_mean_q;
    double *child_window_q;
    uint8_t *child_passed;
};

__device__ __forceinline__ uint8_t cutoffs(const flx_params &p, int L, double mean, double window) {
    bool ok = true;  // src/read.cpp:64-73
    if (p.min_length_set && L < p.min_length) ok = false;
    else if (p.max_length_set && L > p.max_length) ok = false;
    else if (p.min_mean_q_set && mean < p.min_mean_q) ok = false;
    else if (p.min_window_q_set && window < p.min_window_q) ok = false;
    return ok ? 1 : 0;
}

struct Win {  // one sliding-window recurrence (parent or current child)
    int cnt;    // covered bases so far
    double w;   // window quality
    double mn;  // its minimum
};

__device__ __forceinline__ double window_result(const FoldArgs &a, int len, int cnt, double mn) {
    const double mean = 100.0 * (double)cnt / (double)len;
    if (len <= a.ws) return mean;  // src/read.cpp:217-218
    if (mn < a.clamp) mn = 0.0;
    return 100.0 * mn;
}

// ---- the cooperative path (score_kmer_long.hip) ----------------------------------------------------------------------------------
// What the detection counts on the device and the host reads back with a copy it waits for anyway (the coverage plane's size for
// the reads, the number of children for the children): how many long segments there are, and how many 32-position steps they have.
struct KmerLongCounts {
    unsigned long long n;      // long segments
    unsigned long long words;  // their steps of 32 positions: sum of ceil((len - ws) / 32)
};
struct KmerLong {
    bool on = false;            // the path applies to this call (flx_kmer_long_threshold)
    int thr = 0;                // reads and children of at least thr bases are long
    KmerLongCounts *d_reads = nullptr, *d_children = nullptr;  // device counters, zeroed by flx_kmer_long_begin
    uint64_t n_reads_long = 0, n_children_long = 0;            // the totals of this call (for the stage line)
    uint64_t words = 0;
    double t_start = 0.0;
};
__host__ __device__ inline unsigned long long flx_kmer_long_words(int len, int ws) { return len > ws ? ((unsigned long long)(len - ws) + 31ull) >> 5 : 0ull; }

// FLX_KMER_LONG_MIN and the default rule -> kl->on / kl->thr (an invalid value of the switch: FLX_ERR_INVALID)
int flx_kmer_long_threshold(flx_ctx *ctx, uint64_t plane_bytes, bool applies, KmerLong *kl);
// the long reads: word summaries and the cooperative walk (parents' mean_q / window_q / passed); with `children` also n_child of
// every long read and the long children's counts in kl->d_children.  Stream-ordered, no wait.
int flx_kmer_long_reads(flx_ctx *ctx, const FoldArgs &a, KmerLong *kl, const KmerLongCounts &reads, bool children, void *work, size_t work_bytes);
size_t flx_kmer_long_reads_workspace(const KmerLongCounts &reads);
// after the offsets' scan: the long reads' child ranges (child_ranges, child_parent) and the long children's scores
int flx_kmer_long_children(flx_ctx *ctx, const FoldArgs &a, KmerLong *kl, const KmerLongCounts &reads, const KmerLongCounts &children, void *reads_work,
                           void *work, size_t work_bytes);
size_t flx_kmer_long_children_workspace(const KmerLongCounts &children);
// FLX_API_TIMING: the stage line — wall time from the path's first launch to the end of the call's device work, which it waits for
int flx_kmer_long_report(flx_ctx *ctx, const KmerLong &kl, const void *reads_work, const void *children_work);
