// summary.hip — flx_summary(_dev): what a set of reads looks like — entries, bases, shortest, longest, median, N10..N90 and the
// histograms of length, mean quality and window quality — from the per-read arrays the global stage already holds.  Every field
// is an integer and every definition is exact, so N ranks give the bits of one rank.
//
//   pass 0      k_summary_stats streams length, both qualities and the mask once: the three histograms (136 bins of
//               (entries, bases)), n, bases, shortest and longest.  Per-workgroup partials in LDS, one flush of vector atomics
//               per workgroup into a zeroed block of device memory.
//   passes 1-4  k_summary_select: radix selection of the ten order statistics (nine Nx and the median) on the 32-bit length, 8
//               bits per pass from the top.  An entry belongs to at most one of the at most ten distinct prefixes still alive and
//               adds (1, length) to that prefix's 256-bin row in LDS (10 x 256 x 16 B = 40 KiB at most); one flush per workgroup.
//               After each pass the rows come to the host (summed over the ranks when the call is collective), which picks
//               every target's digit: summary_select.h.
// Five small host round trips per call; all accumulators are 64-bit.
// The timing bracket "flx_summary" spans the whole call on the stream — the five kernels, their memsets and copies, the host's
// synchronisation and digit choice between the passes and, in a collective call, the nested exchanges (i.e. the wait for the
// slowest rank) — not the kernels alone.
#include <algorithm>
#include <cmath>

#include "flx_internal.h"
#include "summary_select.h"

namespace {

namespace sel = flx_summary_select;

constexpr int kLenBins = FLX_SUMMARY_LEN_BINS, kQBins = FLX_SUMMARY_Q_BINS;
constexpr int kBins = kLenBins + 2 * kQBins;  // 136: length, mean quality, window quality
constexpr int kEdges = 51;
// the block of 64-bit words pass 0 accumulates into
enum : int {
    W_N = 0,       // entries counted
    W_BASES = 1,   // sum of their lengths
    W_SHORT = 2,   // max over the entries of 2^31 - length (0: no entry), so that a zeroed block is the empty state
    W_LONG = 3,    // max over the entries of length + 1 (0: no entry)
    W_BAD = 4,     // counted entries with a negative length
    W_HIST = 8,    // bin k: entries at W_HIST + 2 k, bases at W_HIST + 2 k + 1
    W_STATS_END = W_HIST + 2 * kBins,
    W_EDGES = 288,                        // the 51 doubles of flx_summary_q_edges
    W_ROWS = 512,                         // the rows of a selection pass: sel::kTargets x 256 x (entries, bases)
    W_END = W_ROWS + sel::kTargets * sel::kDigits * 2,
};
static_assert(W_STATS_END <= W_EDGES && W_EDGES + kEdges <= W_ROWS, "layout");

typedef unsigned long long u64;

// edges[k] = 100 (1 - 10^(-k/10)): the quality (0-100 scale of mean_q / window_q) of Phred k.  Host libm, once; through a volatile
// pointer so that the compiler cannot fold pow(10, x) into another function (as for the Phred table, flx_ctx.hip).
void q_edges(double *e) {
    double (*volatile powfn)(double, double) = pow;
    for (int k = 0; k < kEdges; ++k) e[k] = 100.0 * (1.0 - powfn(10.0, -k / 10.0));
}

// bin k in 0..49: e[k] <= q < e[k+1]; 50: q >= e[50]; 51: NaN and q < 0
__device__ __forceinline__ int q_bin(double q, const double *e) {
    if (!(q >= 0.0)) return kQBins - 1;
    int lo = 0, hi = kEdges;  // the number of edges <= q (e[0] = 0: at least one)
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (e[mid] <= q) lo = mid + 1;
        else hi = mid;
    }
    return lo - 1;
}

__device__ __forceinline__ int len_bin(int32_t len) { return len <= 1 ? 0 : 31 - __clz(len); }

__device__ __forceinline__ u64 wave_sum(u64 v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    return v;
}
__device__ __forceinline__ u64 wave_max(u64 v) {
    for (int o = 32; o > 0; o >>= 1) {
        const u64 w = __shfl_down(v, o);
        v = w > v ? w : v;
    }
    return v;
}

__global__ void __launch_bounds__(sel::kThreads) k_summary_stats(uint64_t n, const int32_t *__restrict__ length,
                                                                 const double *__restrict__ mean_q,
                                                                 const double *__restrict__ window_q,
                                                                 const uint8_t *__restrict__ mask, const double *__restrict__ edges,
                                                                 u64 *__restrict__ out) {
    __shared__ u64 s_hist[2 * kBins];
    __shared__ u64 s_tot[5];
    __shared__ double s_edges[kEdges];
    for (int k = threadIdx.x; k < 2 * kBins; k += blockDim.x) s_hist[k] = 0;
    if (threadIdx.x < 5) s_tot[threadIdx.x] = 0;
    if (threadIdx.x < kEdges) s_edges[threadIdx.x] = edges[threadIdx.x];
    __syncthreads();
    u64 cnt = 0, bases = 0, shortest = 0, longest = 0, bad = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        if (mask && !mask[i]) continue;
        const int32_t len = length[i];
        if (len < 0) {
            ++bad;
            continue;
        }
        const u64 l = (u64)len;
        ++cnt;
        bases += l;
        shortest = max(shortest, (u64)0x80000000ull - l);
        longest = max(longest, l + 1);
        const int b = len_bin(len);
        atomicAdd(&s_hist[2 * b], 1ull);
        atomicAdd(&s_hist[2 * b + 1], l);
        if (mean_q) {
            const int k = kLenBins + q_bin(mean_q[i], s_edges);
            atomicAdd(&s_hist[2 * k], 1ull);
            atomicAdd(&s_hist[2 * k + 1], l);
        }
        if (window_q) {
            const int k = kLenBins + kQBins + q_bin(window_q[i], s_edges);
            atomicAdd(&s_hist[2 * k], 1ull);
            atomicAdd(&s_hist[2 * k + 1], l);
        }
    }
    cnt = wave_sum(cnt);
    bases = wave_sum(bases);
    bad = wave_sum(bad);
    shortest = wave_max(shortest);
    longest = wave_max(longest);
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(&s_tot[W_N], cnt);
        atomicAdd(&s_tot[W_BASES], bases);
        atomicMax(&s_tot[W_SHORT], shortest);
        atomicMax(&s_tot[W_LONG], longest);
        atomicAdd(&s_tot[W_BAD], bad);
    }
    __syncthreads();
    // one flush per workgroup; bins nobody touched cost nothing
    for (int k = threadIdx.x; k < 2 * kBins; k += blockDim.x)
        if (s_hist[k]) atomicAdd(&out[W_HIST + k], s_hist[k]);
    if (threadIdx.x < 5 && s_tot[threadIdx.x]) {
        if (threadIdx.x == W_SHORT || threadIdx.x == W_LONG) atomicMax(&out[threadIdx.x], s_tot[threadIdx.x]);
        else atomicAdd(&out[threadIdx.x], s_tot[threadIdx.x]);
    }
}

struct SelTable {
    uint32_t prefix[sel::kTargets];  // distinct; rows [0, n_rows)
    int n_rows;
    int shift;                       // the digit of this pass is (length >> shift) & 255, the prefix length >> (shift + 8)
};

// dynamic LDS: n_rows * 256 * (entries, bases) = n_rows * 4 KiB
__global__ void __launch_bounds__(sel::kThreads) k_summary_select(uint64_t n, const int32_t *__restrict__ length,
                                                                  const uint8_t *__restrict__ mask, SelTable t,
                                                                  u64 *__restrict__ out) {
    extern __shared__ u64 s_rows[];
    const int words = t.n_rows * sel::kDigits * 2;
    for (int k = threadIdx.x; k < words; k += blockDim.x) s_rows[k] = 0;
    __syncthreads();
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        if (mask && !mask[i]) continue;
        const int32_t len = length[i];
        if (len < 0) continue;
        const uint32_t key = (uint32_t)len;
        const uint32_t pre = (uint32_t)((uint64_t)key >> (t.shift + 8));
        int r = -1;
#pragma unroll
        for (int k = 0; k < sel::kTargets; ++k)
            if (k < t.n_rows && t.prefix[k] == pre) r = k;
        if (r < 0) continue;
        const int slot = (r * sel::kDigits + (int)((key >> t.shift) & 255u)) * 2;
        atomicAdd(&s_rows[slot], 1ull);
        atomicAdd(&s_rows[slot + 1], (u64)key);
    }
    __syncthreads();
    for (int k = threadIdx.x; k < words; k += blockDim.x)
        if (s_rows[k]) atomicAdd(&out[k], s_rows[k]);
}

unsigned grid_for(uint64_t n) {
    const uint64_t b = (n + sel::kThreads - 1) / sel::kThreads;
    return (unsigned)(b < 1 ? 1 : b > (uint64_t)sel::kMaxBlocks ? (uint64_t)sel::kMaxBlocks : b);
}

int summary_run(flx_ctx *ctx, uint64_t n, const int32_t *d_length, const double *d_mean_q, const double *d_window_q,
                const uint8_t *d_mask, int global, struct flx_summary *out) {
    const bool collective = global != 0 && ctx->comm != nullptr;
    const int world = collective ? flx_comm_world(ctx) : 1, rank = collective ? flx_comm_rank(ctx) : 0;
    void *scratch = nullptr, *pinned = nullptr;
    FLX_CHECK(flx_scratch(ctx, (size_t)W_END * 8, &scratch));
    FLX_CHECK(flx_pinned(ctx, (size_t)W_END * 8, &pinned));
    u64 *d = (u64 *)scratch, *h = (u64 *)pinned;
    hipStream_t st = ctx->stream;
    const unsigned grid = grid_for(n);

    flx_time_scope ts(ctx, "flx_summary");
    // ---- pass 0 ----
    q_edges((double *)(h + W_EDGES));
    FLX_HIP(ctx, hipMemsetAsync(d, 0, (size_t)W_STATS_END * 8, st));
    FLX_HIP(ctx, hipMemcpyAsync(d + W_EDGES, h + W_EDGES, kEdges * 8, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_summary_stats, dim3(grid), dim3(sel::kThreads), 0, st, n, d_length, d_mean_q, d_window_q, d_mask,
                       (const double *)(d + W_EDGES), d);
    FLX_HIP(ctx, hipGetLastError());
    FLX_HIP(ctx, hipMemcpyAsync(h, d, (size_t)W_STATS_END * 8, hipMemcpyDeviceToHost, st));
    FLX_HIP(ctx, hipStreamSynchronize(st));
    u64 shortest = h[W_SHORT], longest = h[W_LONG];
    if (collective) {
        // sums only: the shortest and the longest of every rank travel in a slot of their own (all other slots 0)
        std::vector<uint64_t> ex((size_t)W_STATS_END + 2 * (size_t)world, 0);
        for (int k = 0; k < W_STATS_END; ++k) ex[k] = (k == W_SHORT || k == W_LONG) ? 0 : h[k];
        ex[(size_t)W_STATS_END + 2 * (size_t)rank] = shortest;
        ex[(size_t)W_STATS_END + 2 * (size_t)rank + 1] = longest;
        FLX_CHECK(flx_comm_allreduce_u64_host(ctx, ex.data(), ex.size()));
        for (int k = 0; k < W_STATS_END; ++k) h[k] = ex[k];
        shortest = longest = 0;
        for (int r = 0; r < world; ++r) {
            shortest = std::max<u64>(shortest, ex[(size_t)W_STATS_END + 2 * (size_t)r]);
            longest = std::max<u64>(longest, ex[(size_t)W_STATS_END + 2 * (size_t)r + 1]);
        }
    }
    if (h[W_BAD]) return flx_fail(ctx, FLX_ERR_INVALID, "flx_summary: %llu counted entries have a negative length", (u64)h[W_BAD]);
    out->n = h[W_N];
    out->bases = h[W_BASES];
    out->min_length = out->n ? (int32_t)(0x80000000ull - shortest) : 0;
    out->max_length = out->n ? (int32_t)(longest - 1) : 0;
    for (int b = 0; b < kLenBins; ++b) {
        out->len_count[b] = h[W_HIST + 2 * b];
        out->len_bases[b] = h[W_HIST + 2 * b + 1];
    }
    for (int b = 0; b < kQBins; ++b) {
        out->mean_q_count[b] = h[W_HIST + 2 * (kLenBins + b)];
        out->mean_q_bases[b] = h[W_HIST + 2 * (kLenBins + b) + 1];
        out->window_q_count[b] = h[W_HIST + 2 * (kLenBins + kQBins + b)];
        out->window_q_bases[b] = h[W_HIST + 2 * (kLenBins + kQBins + b) + 1];
    }
    if (out->n == 0) return FLX_OK;  // (every rank of a collective call sees the same n)

    // ---- passes 1-4: the ten order statistics ----
    sel::State s;
    sel::init(s, out->n, out->bases);
    while (s.pass < sel::kPasses) {
        SelTable t;
        for (int r = 0; r < sel::kTargets; ++r) t.prefix[r] = r < s.n_rows ? s.row_prefix[r] : 0;
        t.n_rows = s.n_rows;
        t.shift = sel::shift_of(s);
        const size_t bytes = (size_t)s.n_rows * sel::kDigits * sizeof(sel::Bin);
        FLX_HIP(ctx, hipMemsetAsync(d + W_ROWS, 0, bytes, st));
        hipLaunchKernelGGL(k_summary_select, dim3(grid), dim3(sel::kThreads), bytes, st, n, d_length, d_mask, t, d + W_ROWS);
        FLX_HIP(ctx, hipGetLastError());
        FLX_HIP(ctx, hipMemcpyAsync(h + W_ROWS, d + W_ROWS, bytes, hipMemcpyDeviceToHost, st));
        FLX_HIP(ctx, hipStreamSynchronize(st));
        if (collective) FLX_CHECK(flx_comm_allreduce_u64_host(ctx, (uint64_t *)(h + W_ROWS), bytes / 8));
        static_assert(sizeof(sel::Bin) == 16, "a bin is (entries, bases)");
        sel::step(s, (const sel::Bin *)(h + W_ROWS));
    }
    ts.end();
    if (!s.consistent) return flx_fail(ctx, FLX_ERR_STATE, "flx_summary: the arrays changed between the passes");
    for (int x = 0; x < 9; ++x) out->nx[x] = sel::value(s, x);
    out->median_length = sel::value(s, sel::kMedian);
    return FLX_OK;
}

}  // namespace

extern "C" int flx_summary_q_edges(double edges[51]) {
    if (!edges) return FLX_ERR_INVALID;
    q_edges(edges);
    return FLX_OK;
}

extern "C" int flx_summary_dev(flx_ctx *ctx, uint64_t n, const void *d_length, const void *d_mean_q, const void *d_window_q,
                               const void *d_mask, int global, struct flx_summary *out) {
    if (!ctx) return FLX_ERR_INVALID;
    if (!out || (n && !d_length)) return flx_fail(ctx, FLX_ERR_INVALID, "flx_summary: NULL argument");
    memset(out, 0, sizeof *out);
    FLX_HIP(ctx, hipSetDevice(ctx->device));
    return summary_run(ctx, n, (const int32_t *)d_length, (const double *)d_mean_q, (const double *)d_window_q,
                       (const uint8_t *)d_mask, global, out);
}

extern "C" int flx_summary(flx_ctx *ctx, uint64_t n, const int32_t *length, const double *mean_q, const double *window_q,
                           const uint8_t *mask, int global, struct flx_summary *out) {
    if (!ctx) return FLX_ERR_INVALID;
    if (!out || (n && !length)) return flx_fail(ctx, FLX_ERR_INVALID, "flx_summary: NULL argument");
    memset(out, 0, sizeof *out);
    FLX_HIP(ctx, hipSetDevice(ctx->device));
    flx_dbuf d_len, d_mean, d_win, d_mask;
    FLX_CHECK(flx_dalloc(ctx, d_len, n * 4));
    if (mean_q) FLX_CHECK(flx_dalloc(ctx, d_mean, n * 8));
    if (window_q) FLX_CHECK(flx_dalloc(ctx, d_win, n * 8));
    if (mask) FLX_CHECK(flx_dalloc(ctx, d_mask, n));
    if (n) {
        FLX_HIP(ctx, hipMemcpyAsync(d_len.p, length, n * 4, hipMemcpyHostToDevice, ctx->stream));
        if (mean_q) FLX_HIP(ctx, hipMemcpyAsync(d_mean.p, mean_q, n * 8, hipMemcpyHostToDevice, ctx->stream));
        if (window_q) FLX_HIP(ctx, hipMemcpyAsync(d_win.p, window_q, n * 8, hipMemcpyHostToDevice, ctx->stream));
        if (mask) FLX_HIP(ctx, hipMemcpyAsync(d_mask.p, mask, n, hipMemcpyHostToDevice, ctx->stream));
    }
    // (the device arrays are freed on return: summary_run ends synchronised with the stream on every path that launched)
    return summary_run(ctx, n, (const int32_t *)d_len.p, (const double *)d_mean.p, (const double *)d_win.p,
                       (const uint8_t *)d_mask.p, global, out);
}
