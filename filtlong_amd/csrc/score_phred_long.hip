// score_phred_long.hip — Phred scoring of very long reads with many lanes per read, bit-identical to the reference's serial
// folds (src/read.cpp:208-236).
//
// The default Phred kernels fold one read in one lane, strictly left to right, so a read's time grows with its length and gets no
// help from the rest of the chip: a 4 Mbp read is a serial tail of tens of milliseconds.  Reads from a length threshold on
// (flx_launch_score_phred sets it, see flx_phred_long_threshold) are left alone by the batch kernel and scored here, cut into chunks of 1024
// bases that all run in parallel, with the integer-grid algebra of stats.hip (fold_map.h):
//
//   mean fold     s += Q[byte]  (non-negative elements): per chunk an approximate sum, a per-read scan of those (a GUESS of the
//                 binade of s at every chunk start) and the integer parity map of the chunk for that binade.
//   window fold   w = fl(w - D[old]); w = fl(w + D[new]); mn = min(mn, w).  Inside binade E each of the two roundings is a
//                 parity map on the integer M (w = M 2^(E-52)), so a step, and any run of steps, is M -> M + g[M & 1].  A chunk's
//                 summary per entry parity p holds g[p], the minimum offset after full steps (-> mn) and the lowest / highest
//                 offset of every intermediate, half-steps included.  The guess of E comes from the approximate prefix sums.
//   walk          one wave per read carries the EXACT s, then w and mn, through the chunk summaries in order, 64 at a time (an
//                 ordered scan of the summaries, every lane applies its prefix to the entering value, a ballot finds the first
//                 one that does not fit).  A summary is used only if the value really is in the guessed binade and every
//                 intermediate stays at least one grid unit inside it (an exact difference that dips below 2^E would round on the
//                 finer grid).  The chunk that does not fit is opened: lane summaries of 16 bases for the binade the value
//                 really is in, and the lane that does not fit is folded serially, exactly like the reference loop.  Zero,
//                 subnormal, negative or non-finite values and bytes with a negative table value (< 33 or >= 128) always take
//                 the serial path.  A wrong guess costs time, never correctness.
//   finish        the first window is fl(s_ws) / ws, where s_ws is the mean fold's exact prefix at position ws: the walk folds the
//                 chunk that holds position ws serially and records it.  ×100, the clamp and the hard cut-offs go through
//                 finish_read (score_phred_common.h), the same code as the default kernels.
//
// Kernel names all start with flx_score_phred_long; the work after the detection kernel is one timing bracket of that name.
#include <algorithm>
#include <cerrno>
#include <chrono>

#include "flx_internal.h"
#include "fold_map.h"
#include "score_phred_common.h"

using namespace flx_phred;
using namespace flx_fold;

namespace {

constexpr int LANE_EL = 16;             // bases per lane in a chunk
constexpr int CHUNK = 64 * LANE_EL;     // bases per chunk (one wave)
constexpr long long SAT = 1ll << 61;    // offsets saturate here: far outside any binade, and a sum of two never overflows
constexpr long long NOSTEP = 1ll << 62; // WinSum::mf of a run without a full step
constexpr long long M_LO = (1ll << 52) + 1, M_HI = (1ll << 53) - 1;  // the window's range test: one grid unit inside the binade
constexpr int SLOT_BLOCKS = 1024;       // blocks of the stable compaction of the long reads' ids
constexpr int MAX_OPEN = 16;            // lane-summary attempts in an opened chunk before the rest of it is folded serially ...
constexpr int MAX_STALL = 2;            // ... or attempts that fitted fewer than MIN_ADVANCE lanes (a value that hovers at a
constexpr int MIN_ADVANCE = 4;          // binade boundary: a lane summary costs ~30 serial steps)

__device__ __forceinline__ long long sat(long long x) { return x > SAT ? SAT : x < -SAT ? -SAT : x; }
// c ? x1 : x0 as bit arithmetic: a plain select of two struct members by parity is turned into an indexed load from the stack
__device__ __forceinline__ long long sel(bool c, long long x1, long long x0) { return x0 ^ ((x0 ^ x1) & -(long long)c); }

__device__ __forceinline__ Map2 compose_sat(const Map2 &a, const Map2 &b) {  // compose() with saturation (elements >= 0)
    Map2 c;
    c.a0 = sat(a.a0 + sel((a.a0 & 1) != 0, b.a1, b.a0));
    c.a1 = sat(a.a1 + sel(((1 + a.a1) & 1) != 0, b.a1, b.a0));
    return c;
}

// double with unbiased exponent e and integer significand M in [2^52, 2^53] (2^53 is 2^(e+1))
__device__ __forceinline__ double make_f64(int e, long long M) {
    return __longlong_as_double((long long)(((unsigned long long)(e + 1023) << 52) + (unsigned long long)(M - (1ll << 52))));
}
__device__ __forceinline__ long long significand(double v) {
    return (long long)(((unsigned long long)__double_as_longlong(v) & 0x000fffffffffffffull) | (1ull << 52));
}
__device__ __forceinline__ long long readlane_i64(long long v, int src) {
    const unsigned int lo = (unsigned int)__builtin_amdgcn_readlane((int)(v & 0xffffffffll), src);
    const unsigned int hi = (unsigned int)__builtin_amdgcn_readlane((int)(v >> 32), src);
    return (long long)(((unsigned long long)hi << 32) | lo);
}

// ---------------------------------------------------------------------------------------------------- window-step summaries
struct WinSum {
    long long g[2];   // end offset for entry parity p
    long long mf[2];  // minimum offset after a full step (NOSTEP: none)
    long long lo[2];  // lowest / highest offset of every intermediate, the entry (0) included
    long long hi[2];
};
__device__ __forceinline__ WinSum win_identity() {
    WinSum s;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        s.g[p] = 0;
        s.mf[p] = NOSTEP;
        s.lo[p] = 0;
        s.hi[p] = 0;
    }
    return s;
}
__device__ __forceinline__ WinSum win_compose(const WinSum &A, const WinSum &B) {  // A first, then B
    WinSum C;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const bool q = ((p + (int)(A.g[p] & 1)) & 1) != 0;  // selects, not a runtime index: the summaries stay in registers
        const long long bg = sel(q, B.g[1], B.g[0]), bmf = sel(q, B.mf[1], B.mf[0]);
        const long long blo = sel(q, B.lo[1], B.lo[0]), bhi = sel(q, B.hi[1], B.hi[0]);
        C.g[p] = sat(A.g[p] + bg);
        C.mf[p] = bmf == NOSTEP ? A.mf[p] : min(A.mf[p], sat(A.g[p] + bmf));
        C.lo[p] = min(A.lo[p], sat(A.g[p] + blo));
        C.hi[p] = max(A.hi[p], sat(A.g[p] + bhi));
    }
    return C;
}
// one window step in binade E: w - d_old, then + d_new (both >= 0; ok = false if either cannot be applied inside the binade)
__device__ __forceinline__ WinSum win_step(double d_old, double d_new, int E, bool &ok) {
    const Map2 s = elem_map(d_old, E, ok), a = elem_map(d_new, E, ok);
    WinSum r;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const long long o1 = -(p ? s.a1 : s.a0);
        const bool p1 = ((p + (int)(o1 & 1)) & 1) != 0;
        const long long o2 = o1 + sel(p1, a.a1, a.a0);
        r.g[p] = o2;
        r.mf[p] = o2;
        r.lo[p] = min(0ll, min(o1, o2));
        r.hi[p] = max(0ll, max(o1, o2));
    }
    return r;
}
__device__ __forceinline__ WinSum win_shfl_up(const WinSum &s, int o) {
    WinSum r;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        r.g[p] = __shfl_up(s.g[p], o, 64);
        r.mf[p] = __shfl_up(s.mf[p], o, 64);
        r.lo[p] = __shfl_up(s.lo[p], o, 64);
        r.hi[p] = __shfl_up(s.hi[p], o, 64);
    }
    return r;
}
__device__ __forceinline__ WinSum win_shfl_down(const WinSum &s, int o) {
    WinSum r;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        r.g[p] = __shfl_down(s.g[p], o, 64);
        r.mf[p] = __shfl_down(s.mf[p], o, 64);
        r.lo[p] = __shfl_down(s.lo[p], o, 64);
        r.hi[p] = __shfl_down(s.hi[p], o, 64);
    }
    return r;
}

struct MeanMeta {
    long long a0, a1;
    int e;  // guessed binade of s, or NO_MAP
    int pad;
};
struct WinMeta {
    WinSum s;
    int e;  // guessed binade of w, or NO_MAP
    int pad;
};

struct LongArgs {
    PhredArgs a;               // plane, offsets, lengths, tables, ws, clamp, cut-offs, outputs
    const uint32_t *ids;       // [k] the long reads (read ids, in processing order)
    uint32_t k;
    const uint32_t *mbase;     // [k + 1] first mean chunk of each long read
    const uint32_t *wbase;     // [k + 1] first window chunk
    uint32_t *m_read;          // [n_mean] long-read index of every mean chunk
    uint32_t *w_read;          // [n_win]
    uint32_t n_mean, n_win;
    double *csum, *cstart, *chead;  // [n_mean] approximate sum, approximate prefix at the start, sum of the first ws % CHUNK bases
    unsigned char *clean;      // [n_mean] every byte has a non-negative table value
    MeanMeta *mmeta;           // [n_mean]
    WinMeta *wmeta;            // [n_win]
};

__device__ __forceinline__ bool nonneg_byte(uint32_t b) { return b >= 33 && b < 128; }  // Q[b] >= 0 (read.cpp:270-273)

__device__ __forceinline__ void load_tables(const PhredArgs &a, double *lq, double *ld) {
    for (int i = threadIdx.x; i < 257; i += blockDim.x) {
        lq[i] = a.lut_q[i];
        ld[i] = a.lut_d[i];
    }
    __syncthreads();
}

// the 16 bytes of a lane at position pos (a multiple of 16) of a read of length L; bytes at or beyond L are 0 (not used)
__device__ __forceinline__ uint4 load16(const uint8_t *q, long long pos, int L) {
    if (pos >= L) return make_uint4(0, 0, 0, 0);
    return *reinterpret_cast<const uint4 *>(q + pos);  // inside the read's 16-byte padded span
}

// ---------------------------------------------------------------------------------------------------- detection and compaction
// Counts, per length bucket (bucket b: lengths from t0 << b; one bucket when the threshold is given), the reads, their mean and
// window chunks.  Layout of `out`: n[NB], mean chunks[NB], window chunks[NB].  Global atomics only for long reads: a batch without
// any costs one pass over the lengths.
__global__ void __launch_bounds__(256) flx_score_phred_long_find(const int32_t *lengths, uint64_t n, int ws, int t0, int nb,
                                                                 unsigned long long *out) {
    __shared__ unsigned long long sh[3 * PHRED_LONG_NB];
    for (int i = threadIdx.x; i < 3 * PHRED_LONG_NB; i += 256) sh[i] = 0;
    __syncthreads();
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t i0 = (uint64_t)blockIdx.x * 256 + threadIdx.x; i0 < n; i0 += 4 * stride) {
        int Ls[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) Ls[u] = i0 + u * stride < n ? lengths[i0 + u * stride] : 0;  // four loads in flight
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int L = Ls[u];
            if (L >= t0) {
                int b = 0;
                if (nb > 1) b = min(nb - 1, (31 - __clz(L)) - (31 - __clz(t0)));
                atomicAdd(&sh[b], 1ull);
                atomicAdd(&sh[PHRED_LONG_NB + b], (unsigned long long)((L + CHUNK - 1) / CHUNK));
                if (L > ws) atomicAdd(&sh[2 * PHRED_LONG_NB + b], (unsigned long long)((L - ws + CHUNK - 1) / CHUNK));
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 3 * PHRED_LONG_NB; i += 256)
        if (sh[i]) atomicAdd(&out[i], sh[i]);
}

// long reads per block of the processing order (block b: slots [b per, (b + 1) per))
__global__ void __launch_bounds__(256) flx_score_phred_long_count(const int32_t *lengths, const uint32_t *order, uint64_t n,
                                                                  uint64_t per, int thr, uint32_t *blk) {
    const uint64_t s0 = (uint64_t)blockIdx.x * per, s1 = min(n, s0 + per);
    int c = 0;
    for (uint64_t t = s0; t < s1; t += 256) {
        const uint64_t slot = t + threadIdx.x;
        bool f = false;
        if (slot < s1) f = lengths[order ? order[slot] : (uint32_t)slot] >= thr;
        c += __syncthreads_count(f);
    }
    if (threadIdx.x == 0) blk[blockIdx.x] = (uint32_t)c;
}

// exclusive scan of n 64-bit values by one block of 1024 threads; out[n] = total
__device__ void block_exclusive_scan(const unsigned long long *in, unsigned long long *out, uint64_t n) {
    __shared__ unsigned long long wsum[16];
    __shared__ unsigned long long carry;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (uint64_t t = 0; t < n; t += 1024) {
        const uint64_t i = t + threadIdx.x;
        const unsigned long long v = i < n ? in[i] : 0;
        unsigned long long x = v;
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned long long y = __shfl_up(x, o, 64);
            if (lane >= o) x += y;
        }
        if (lane == 63) wsum[wave] = x;
        __syncthreads();
        unsigned long long before = carry;
        for (int w = 0; w < wave; ++w) before += wsum[w];
        if (i < n) out[i] = before + x - v;
        __syncthreads();
        if (threadIdx.x == 1023) carry = before + x;
        __syncthreads();
    }
    if (threadIdx.x == 0) out[n] = carry;
}

// stable compaction of the processing order: the long reads' ids, in order (blk: the counts of flx_score_phred_long_count)
__global__ void __launch_bounds__(256) flx_score_phred_long_compact(const int32_t *lengths, const uint32_t *order, uint64_t n,
                                                                    uint64_t per, int thr, const uint32_t *blk, uint32_t *ids) {
    __shared__ uint32_t wcount[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t c = 0;  // long reads before this block
    for (uint32_t i = threadIdx.x; i < blockIdx.x; i += 256) c += blk[i];
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if (lane == 0) wcount[wave] = c;
    __syncthreads();
    uint64_t nl = (uint64_t)wcount[0] + wcount[1] + wcount[2] + wcount[3];
    const uint64_t s0 = (uint64_t)blockIdx.x * per, s1 = min(n, s0 + per);
    for (uint64_t t = s0; t < s1; t += 256) {
        const uint64_t slot = t + threadIdx.x;
        uint32_t rid = 0;
        bool f = false;
        if (slot < s1) {
            rid = order ? order[slot] : (uint32_t)slot;
            f = lengths[rid] >= thr;
        }
        const unsigned long long m = __ballot(f);
        __syncthreads();  // (the previous tile's counts have been read)
        if (lane == 0) wcount[wave] = (uint32_t)__popcll(m);
        __syncthreads();
        uint32_t before = 0, tile = 0;
        for (int w = 0; w < 4; ++w) {
            if (w < wave) before += wcount[w];
            tile += wcount[w];
        }
        if (f) ids[nl + before + __popcll(m & ((1ull << lane) - 1ull))] = rid;
        nl += tile;
    }
}

// per long read: first mean / window chunk (exclusive scans of the chunk counts, both in one 64-bit word)
__global__ void __launch_bounds__(1024) flx_score_phred_long_index(const PhredArgs a, const uint32_t *ids, uint32_t k,
                                                                   unsigned long long *tmp, uint32_t *mbase, uint32_t *wbase) {
    for (uint32_t i = threadIdx.x; i < k; i += 1024) {
        const int L = a.lengths[ids[i]];
        const unsigned long long nm = (unsigned long long)((L + CHUNK - 1) / CHUNK);
        const unsigned long long nw = L > a.ws ? (unsigned long long)((L - a.ws + CHUNK - 1) / CHUNK) : 0ull;
        tmp[i] = nm | (nw << 32);
    }
    __syncthreads();
    block_exclusive_scan(tmp, tmp + k + 1, k);
    __syncthreads();
    for (uint32_t i = threadIdx.x; i <= k; i += 1024) {
        const unsigned long long v = tmp[k + 1 + i];
        mbase[i] = (uint32_t)v;
        wbase[i] = (uint32_t)(v >> 32);
    }
}

// chunk -> long read
__global__ void __launch_bounds__(256) flx_score_phred_long_expand(const LongArgs g) {
    const int lane = threadIdx.x & 63;
    for (uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6); i < g.k; i += gridDim.x * 4) {
        for (uint32_t c = g.mbase[i] + lane; c < g.mbase[i + 1]; c += 64) g.m_read[c] = i;
        for (uint32_t c = g.wbase[i] + lane; c < g.wbase[i + 1]; c += 64) g.w_read[c] = i;
    }
}

// ---------------------------------------------------------------------------------------------------- chunk summaries
// approximate sum of every mean chunk (any order), the sum of its first ws % CHUNK bases, and whether it is clean
__global__ void __launch_bounds__(256) flx_score_phred_long_sums(const LongArgs g) {
    __shared__ double lq[LUT_PAD], ld[LUT_PAD];
    load_tables(g.a, lq, ld);
    const int lane = threadIdx.x & 63;
    const uint32_t c = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c >= g.n_mean) return;
    const uint32_t i = g.m_read[c];
    const uint32_t rid = g.ids[i];
    const int L = g.a.lengths[rid];
    const uint8_t *q = g.a.plane + g.a.offsets[rid];
    const long long pos0 = (long long)(c - g.mbase[i]) * CHUNK + lane * LANE_EL;
    const int h = g.a.ws % CHUNK;
    const uint4 v = load16(q, pos0, L);
    double acc = 0.0, head = 0.0;
    bool clean = true;
#pragma unroll
    for (int j = 0; j < LANE_EL; ++j) {
        if (pos0 + j < L) {
            const uint32_t b = byte_of(v, j);
            const double x = lq[b];
            acc += x;
            if (lane * LANE_EL + j < h) head += x;
            clean = clean && nonneg_byte(b);
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        acc += __shfl_xor(acc, o, 64);
        head += __shfl_xor(head, o, 64);
    }
    const bool all_clean = __all(clean);
    if (lane == 0) {
        g.csum[c] = acc;
        g.chead[c] = head;
        g.clean[c] = all_clean ? 1 : 0;
    }
}

// approximate running sum at every mean chunk start: one wave per long read
__global__ void __launch_bounds__(64) flx_score_phred_long_prefix(const LongArgs g) {
    const int lane = threadIdx.x;
    const uint32_t i = blockIdx.x;
    double carry = 0.0;
    for (uint32_t c0 = g.mbase[i]; c0 < g.mbase[i + 1]; c0 += 64) {
        const uint32_t c = c0 + lane;
        const double v = c < g.mbase[i + 1] ? g.csum[c] : 0.0;
        double x = v;
        for (int o = 1; o < 64; o <<= 1) {
            const double y = __shfl_up(x, o, 64);
            if (lane >= o) x += y;
        }
        if (c < g.mbase[i + 1]) g.cstart[c] = carry + (x - v);
        carry += readlane_f64(x, 63);
    }
}

// the chunk maps: waves [0, n_mean) the mean fold, [n_mean, n_mean + n_win) the window fold
__global__ void __launch_bounds__(256) flx_score_phred_long_maps(const LongArgs g) {
    __shared__ double lq[LUT_PAD], ld[LUT_PAD];
    load_tables(g.a, lq, ld);
    const int lane = threadIdx.x & 63;
    const uint32_t wv = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int ws = g.a.ws;
    if (wv < g.n_mean) {
        const uint32_t c = wv;
        const uint32_t i = g.m_read[c];
        const uint32_t rid = g.ids[i];
        const int L = g.a.lengths[rid];
        const uint32_t cl = c - g.mbase[i];
        const uint8_t *q = g.a.plane + g.a.offsets[rid];
        // guess the binade from the approximate running sum at the chunk's start and end
        const double p0 = g.cstart[c] * (1.0 - 1e-9);
        const double p1 = (g.cstart[c] + g.csum[c]) * (1.0 + 1e-9);
        int e = NO_MAP;
        if (g.clean[c] && p0 > 2.3e-308 && p1 < 1e300 && exponent_of(p0) == exponent_of(p1)) e = exponent_of(p0);
        if (L > ws && cl == (uint32_t)(ws / CHUNK)) e = NO_MAP;  // the walk records the first window's sum inside this chunk
        Map2 m;
        m.a0 = m.a1 = 0;
        bool ok = true;
        if (e != NO_MAP) {
            const long long pos0 = (long long)cl * CHUNK + lane * LANE_EL;
            const uint4 v = load16(q, pos0, L);
#pragma unroll
            for (int j = 0; j < LANE_EL; ++j)
                if (pos0 + j < L) m = compose_sat(m, elem_map(lq[byte_of(v, j)], e, ok));
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {  // ordered wave reduction (lane order == base order)
                Map2 nb;
                nb.a0 = __shfl_down(m.a0, o, 64);
                nb.a1 = __shfl_down(m.a1, o, 64);
                if ((lane & (2 * o - 1)) == 0) m = compose_sat(m, nb);
            }
            if (!__all(ok)) e = NO_MAP;
        }
        if (lane == 0) {
            MeanMeta mm;
            mm.a0 = m.a0;
            mm.a1 = m.a1;
            mm.e = e;
            mm.pad = 0;
            g.mmeta[c] = mm;
        }
    } else if (wv < g.n_mean + g.n_win) {
        const uint32_t c = wv - g.n_mean;
        const uint32_t i = g.w_read[c];
        const uint32_t rid = g.ids[i];
        const int L = g.a.lengths[rid];
        const uint32_t cl = c - g.wbase[i];
        const uint8_t *q = g.a.plane + g.a.offsets[rid];
        // approximate window before the chunk's first step t0 = cl * CHUNK: (P(t0 + ws) - P(t0)) / ws; t0 is a mean chunk start and
        // t0 + ws lies ws % CHUNK bases into mean chunk cl + ws / CHUNK
        const uint32_t mb = g.mbase[i];
        const uint32_t cn = mb + cl + (uint32_t)(ws / CHUNK);
        const double wa = (g.cstart[cn] + g.chead[cn] - g.cstart[mb + cl]) / g.a.ws_d;
        int e = NO_MAP;
        if (wa > 2.3e-308 && wa < 1e300) e = exponent_of(wa);
        WinSum s = win_identity();
        bool ok = true;
        if (e != NO_MAP) {
            const long long n_steps = (long long)L - ws;
            const long long t0 = (long long)cl * CHUNK + lane * LANE_EL;
            const uint4 vo = load16(q, t0, L);
#pragma unroll
            for (int j = 0; j < LANE_EL; ++j) {
                const long long t = t0 + j;
                if (t < n_steps) {
                    const double d_old = ld[byte_of(vo, j)], d_new = ld[q[t + ws]];
                    ok = ok && d_old >= 0.0 && d_new >= 0.0;
                    s = win_compose(s, win_step(d_old, d_new, e, ok));
                }
            }
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const WinSum nb = win_shfl_down(s, o);
                if ((lane & (2 * o - 1)) == 0) s = win_compose(s, nb);
            }
            if (!__all(ok)) e = NO_MAP;
        }
        if (lane == 0) {
            WinMeta wm;
            wm.s = s;
            wm.e = e;
            wm.pad = 0;
            g.wmeta[c] = wm;
        }
    }
}

// ---------------------------------------------------------------------------------------------------- the walk
// Applies the maps of lanes start, start + 1, ... to S (positive, normal, in binade e) for as long as they are usable and S stays in
// the binade, all at once (stats.hip: wave_apply_prefix).  Returns the first lane NOT applied (64: all were).
__device__ __forceinline__ int mean_apply_prefix(double &S, int e, Map2 m, bool usable, int start, int lane) {
    const unsigned long long bad = __ballot(lane >= start && !usable);
    const int first_bad = bad ? (int)__ffsll((long long)bad) - 1 : 64;
    if (lane < start || lane >= first_bad) m.a0 = m.a1 = 0;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        Map2 prev;
        prev.a0 = __shfl_up(m.a0, o, 64);
        prev.a1 = __shfl_up(m.a1, o, 64);
        if (lane >= o) m = compose_sat(prev, m);
    }
    const long long ms = significand(S);
    const long long m2 = ms + sel((ms & 1) != 0, m.a1, m.a0);
    const bool inside = m2 <= (1ll << 53);  // elements >= 0: reaching 2^(e+1) exactly is still on this binade's grid
    const unsigned long long out = __ballot(lane >= start && lane < first_bad && !inside);
    const int f = out ? (int)__ffsll((long long)out) - 1 : first_bad;
    if (f > start) S = make_f64(e, readlane_i64(m2, f - 1));
    return f;
}

// the same for the window: w (positive, normal) and mn advance through the summaries of lanes start, ... while every intermediate
// stays within [2^52 + 1, 2^53 - 1] of w's binade
__device__ __forceinline__ int win_apply_prefix(double &w, double &mn, WinSum s, bool usable, int start, int lane) {
    const int e = exponent_of(w);
    const unsigned long long bad = __ballot(lane >= start && !usable);
    const int first_bad = bad ? (int)__ffsll((long long)bad) - 1 : 64;
    if (lane < start || lane >= first_bad) s = win_identity();
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const WinSum prev = win_shfl_up(s, o);
        if (lane >= o) s = win_compose(prev, s);
    }
    const long long M = significand(w);
    const bool p = (M & 1) != 0;
    const bool inside = M + sel(p, s.lo[1], s.lo[0]) >= M_LO && M + sel(p, s.hi[1], s.hi[0]) <= M_HI;
    const unsigned long long out = __ballot(lane >= start && lane < first_bad && !inside);
    const int f = out ? (int)__ffsll((long long)out) - 1 : first_bad;
    if (f > start) {
        const long long gg = readlane_i64(sel(p, s.g[1], s.g[0]), f - 1);
        const long long mf = readlane_i64(sel(p, s.mf[1], s.mf[0]), f - 1);
        w = make_f64(e, M + gg);
        if (mf != NOSTEP) {
            const double c = make_f64(e, M + mf);
            if (c < mn) mn = c;
        }
    }
    return f;
}

// one wave per long read: the exact mean fold (recording the first window's sum), then the exact window fold
__global__ void __launch_bounds__(64) flx_score_phred_long_walk(const LongArgs g) {
    __shared__ double lq[LUT_PAD], ld[LUT_PAD];
    __shared__ double open_old[CHUNK], open_new[CHUNK];  // the values of an opened chunk, read back at one address by the whole wave
    load_tables(g.a, lq, ld);
    const int lane = threadIdx.x;
    const uint32_t i = blockIdx.x;
    const uint32_t rid = g.ids[i];
    const int L = g.a.lengths[rid];
    const int ws = g.a.ws;
    const uint8_t *q = g.a.plane + g.a.offsets[rid];

    // ---- mean fold
    double S = 0.0, s_ws = 0.0;
    const uint32_t mb = g.mbase[i], nm = g.mbase[i + 1] - mb;
    const int fc = L > ws ? ws / CHUNK : -1;  // the chunk that holds position ws
    for (uint32_t cb = 0; cb < nm; cb += 64) {
        MeanMeta mm;
        mm.a0 = mm.a1 = 0;
        mm.e = NO_MAP;
        if (cb + lane < nm) mm = g.mmeta[mb + cb + lane];
        const int cnt = (int)min<uint32_t>(64, nm - cb);
        int cs = 0;
        while (cs < cnt) {
            int f = cs;
            if (normal_positive(S)) {
                const int e = exponent_of(S);
                Map2 m;
                m.a0 = mm.a0;
                m.a1 = mm.a1;
                f = mean_apply_prefix(S, e, m, lane < cnt && mm.e == e, cs, lane);
            }
            if (f >= cnt) break;
            // chunk cb + f does not apply: open it (lane l holds bases [16 l, 16 l + 16) of it)
            const int cl = (int)cb + f;
            const long long pos0 = (long long)cl * CHUNK;
            const uint4 v = load16(q, pos0 + lane * LANE_EL, L);
            double x[LANE_EL];
            bool ok = true;
#pragma unroll
            for (int j = 0; j < LANE_EL; ++j) {
                const bool in = pos0 + lane * LANE_EL + j < L;
                const uint32_t b = byte_of(v, j);
                x[j] = in ? lq[b] : 0.0;
                ok = ok && (!in || nonneg_byte(b));
            }
            const int m_el = (int)min<long long>(CHUNK, L - pos0);
            const int n_lanes = (m_el + LANE_EL - 1) / LANE_EL;
            const int lws = cl == fc ? (int)((ws - pos0) / LANE_EL) : -1;
            __syncthreads();  // (the previous opened chunk has been read)
#pragma unroll
            for (int j = 0; j < LANE_EL; ++j) open_new[lane * LANE_EL + j] = x[j];
            __syncthreads();
            int ls = 0, opened = 0, stalled = 0;
            while (ls < n_lanes) {
                int fl = ls;
                // the first chunk climbs through a binade every few bases, and a chunk that keeps failing is not worth more scans
                if (cl != 0 && opened < MAX_OPEN && normal_positive(S)) {
                    const int e = exponent_of(S);
                    Map2 m;
                    m.a0 = m.a1 = 0;
                    bool lok = ok;
#pragma unroll
                    for (int j = 0; j < LANE_EL; ++j)
                        if (lane * LANE_EL + j < m_el) m = compose_sat(m, elem_map(x[j], e, lok));
                    fl = mean_apply_prefix(S, e, m, lok && lane < n_lanes && lane != lws, ls, lane);
                    if (fl - ls < MIN_ADVANCE) ++stalled;  // few lanes fitted: summaries are not worth their cost here
                }
                if (fl >= n_lanes) break;
                // serial, base by base, exactly like the reference loop (the values are loaded ahead of the dependent chain)
                double v[LANE_EL];
#pragma unroll
                for (int j = 0; j < LANE_EL; ++j) v[j] = open_new[fl * LANE_EL + j];
#pragma unroll
                for (int j = 0; j < LANE_EL; ++j) {
                    const long long pos = pos0 + fl * LANE_EL + j;
                    if (pos < L) {
                        if (pos == ws) s_ws = S;
                        S += v[j];
                    }
                }
                opened += stalled >= MAX_STALL ? MAX_OPEN : 1;
                ls = fl + 1;
            }
            cs = f + 1;
        }
    }

    // ---- window fold
    double mn = 0.0;
    if (L > ws) {
        double w = s_ws / g.a.ws_d;  // src/read.cpp:223
        mn = w;
        const uint32_t wb = g.wbase[i], nw = g.wbase[i + 1] - wb;
        const long long n_steps = (long long)L - ws;
        for (uint32_t cb = 0; cb < nw; cb += 64) {
            WinMeta wm;
            wm.s = win_identity();
            wm.e = NO_MAP;
            if (cb + lane < nw) wm = g.wmeta[wb + cb + lane];
            const int cnt = (int)min<uint32_t>(64, nw - cb);
            int cs = 0;
            while (cs < cnt) {
                int f = cs;
                if (normal_positive(w)) f = win_apply_prefix(w, mn, wm.s, lane < cnt && wm.e == exponent_of(w), cs, lane);
                if (f >= cnt) break;
                // window chunk cb + f does not apply: open it (lane l holds steps [16 l, 16 l + 16) of it)
                const long long t0 = (long long)(cb + f) * CHUNK;
                const uint4 vo = load16(q, t0 + lane * LANE_EL, L);
                double d_old[LANE_EL], d_new[LANE_EL];
                bool ok = true;
#pragma unroll
                for (int j = 0; j < LANE_EL; ++j) {
                    const long long t = t0 + lane * LANE_EL + j;
                    const bool in = t < n_steps;
                    d_old[j] = in ? ld[byte_of(vo, j)] : 0.0;
                    d_new[j] = in ? ld[q[t + ws]] : 0.0;
                    ok = ok && d_old[j] >= 0.0 && d_new[j] >= 0.0;
                }
                const int m_el = (int)min<long long>(CHUNK, n_steps - t0);
                const int n_lanes = (m_el + LANE_EL - 1) / LANE_EL;
                __syncthreads();
#pragma unroll
                for (int j = 0; j < LANE_EL; ++j) {
                    open_old[lane * LANE_EL + j] = d_old[j];
                    open_new[lane * LANE_EL + j] = d_new[j];
                }
                __syncthreads();
                int ls = 0, opened = 0, stalled = 0;
                while (ls < n_lanes) {
                    int fl = ls;
                    if (opened < MAX_OPEN && normal_positive(w)) {
                        const int e = exponent_of(w);
                        WinSum s = win_identity();
                        bool lok = ok;
#pragma unroll
                        for (int j = 0; j < LANE_EL; ++j)
                            if (lane * LANE_EL + j < m_el) s = win_compose(s, win_step(d_old[j], d_new[j], e, lok));
                        fl = win_apply_prefix(w, mn, s, lok && lane < n_lanes, ls, lane);
                        if (fl - ls < MIN_ADVANCE) ++stalled;
                    }
                    if (fl >= n_lanes) break;
                    double vo[LANE_EL], vn[LANE_EL];
#pragma unroll
                    for (int j = 0; j < LANE_EL; ++j) {
                        vo[j] = open_old[fl * LANE_EL + j];
                        vn[j] = open_new[fl * LANE_EL + j];
                    }
                    if (t0 + (fl + 1) * LANE_EL <= n_steps) {  // a whole lane: no test per step
#pragma unroll
                        for (int j = 0; j < LANE_EL; ++j) {
                            w -= vo[j];          // src/read.cpp:228
                            w += vn[j];          // src/read.cpp:229
                            mn = fmin(mn, w);    // src/read.cpp:230-231 (no NaN here; the sign of a zero minimum is irrelevant)
                        }
                    } else {
                        for (int j = 0; t0 + fl * LANE_EL + j < n_steps; ++j) {
                            w -= vo[j];
                            w += vn[j];
                            mn = fmin(mn, w);
                        }
                    }
                    opened += stalled >= MAX_STALL ? MAX_OPEN : 1;
                    ls = fl + 1;
                }
                cs = f + 1;
            }
        }
    }
    if (lane == 0) finish_read(g.a, rid, L, S, mn);
}

size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }

}  // namespace

// ---------------------------------------------------------------------------------------------------- host side
int flx_phred_long_detect(flx_ctx *ctx, const PhredArgs &a, uint64_t plane_bytes, PhredLong *lp) {
    *lp = PhredLong();
    lp->plane_bytes = plane_bytes;
    long long t0 = PHRED_LONG_FLOOR;
    const char *env = getenv("FLX_PHRED_LONG_MIN");  // test hook: "0" = off; N = every read of >= N bases takes this path
    if (env) {
        char *end = nullptr;
        errno = 0;
        const unsigned long long v = strtoull(env, &end, 10);
        if (!*env || *end || errno || env[0] == '-' || env[0] == '+' || env[0] == ' ')
            return flx_fail(ctx, FLX_ERR_INVALID, "FLX_PHRED_LONG_MIN=%s: expected a non-negative integer (bases)", env);
        if (v == 0 || v > 0x7fffffffull) return FLX_OK;  // off (no read is that long)
        t0 = (long long)v;
        lp->forced = true;
    }
    void *w;
    FLX_CHECK(flx_workspace(ctx, 3, 4096, &w));
    lp->d_counts = (unsigned long long *)w;
    lp->t0 = (int)t0;
    FLX_HIP(ctx, hipMemsetAsync(w, 0, 3 * PHRED_LONG_NB * sizeof(unsigned long long), ctx->stream));
    const unsigned grid = (unsigned)std::min<uint64_t>((a.n_reads + 255) / 256, 2048);
    hipLaunchKernelGGL(flx_score_phred_long_find, dim3(grid), dim3(256), 0, ctx->stream, a.lengths, a.n_reads, a.ws, (int)t0,
                       lp->forced ? 1 : PHRED_LONG_NB, lp->d_counts);
    FLX_HIP(ctx, hipGetLastError());
    lp->on = true;
    return FLX_OK;
}

// Threshold: reads of at least `thr` bases take the cooperative path.  thr starts at the floor (2^18 bases) and doubles while the
// batch's bases per lane of the default kernels (one lane per read, 16 waves of 64 lanes per CU) are at least twice as many: a
// read no longer than a lane's share of the batch finishes inside the batch's time anyway.  The plane's size stands for the bases
// (16-byte padding per read included: an upper bound, so at worst a read stays in the batch that could have left it).
long long flx_phred_long_threshold(const flx_ctx *ctx, const PhredLong *lp, int *b0_out) {
    int b0 = 0;
    long long thr = 0x7fffffff;
    if (lp && lp->on) {
        thr = lp->t0;
        if (!lp->forced) {
            const double per_lane = (double)lp->plane_bytes / ((double)ctx->prop.multiProcessorCount * 1024.0);
            while (b0 + 1 < PHRED_LONG_NB && (double)(thr * 2) <= per_lane) {
                thr *= 2;
                ++b0;
            }
        }
    }
    if (b0_out) *b0_out = b0;
    return thr;
}

int flx_phred_long_score(flx_ctx *ctx, const PhredArgs &a, const PhredLong &lp, const unsigned long long *h, bool *scored) {
    *scored = false;
    if (!lp.on) return FLX_OK;
    int b0 = 0;
    const long long thr = flx_phred_long_threshold(ctx, &lp, &b0);
    unsigned long long k = 0, n_mean = 0, n_win = 0;
    for (int b = b0; b < PHRED_LONG_NB; ++b) {
        k += h[b];
        n_mean += h[PHRED_LONG_NB + b];
        n_win += h[2 * PHRED_LONG_NB + b];
    }
    if (k == 0) return FLX_OK;
    if (n_mean + n_win >= 0xffffffffull)
        return flx_fail(ctx, FLX_ERR_INVALID, "%llu long reads of %llu chunks: too many for one batch", k, n_mean + n_win);
    const bool report = getenv("FLX_API_TIMING") != nullptr;
    const double t_start = std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();

    const uint64_t n = a.n_reads;
    const uint32_t G = (uint32_t)std::min<uint64_t>(SLOT_BLOCKS, (n + 1023) / 1024);
    const uint64_t per = (n + G - 1) / G;
    size_t off = 4096;  // the counts
    const size_t o_blk = off; off = up256(off + (size_t)G * 4);
    const size_t o_tmp = off; off = up256(off + 2 * (k + 1) * 8);
    const size_t o_ids = off; off = up256(off + k * 4);
    const size_t o_mbase = off; off = up256(off + (k + 1) * 4);
    const size_t o_wbase = off; off = up256(off + (k + 1) * 4);
    const size_t o_mread = off; off = up256(off + n_mean * 4);
    const size_t o_wread = off; off = up256(off + n_win * 4 + 4);
    const size_t o_csum = off; off = up256(off + n_mean * 8);
    const size_t o_cstart = off; off = up256(off + n_mean * 8);
    const size_t o_chead = off; off = up256(off + n_mean * 8);
    const size_t o_clean = off; off = up256(off + n_mean);
    const size_t o_mmeta = off; off = up256(off + n_mean * sizeof(MeanMeta));
    const size_t o_wmeta = off; off = up256(off + n_win * sizeof(WinMeta) + 16);
    void *wsp;
    FLX_CHECK(flx_workspace(ctx, 3, off, &wsp));
    char *base = (char *)wsp;

    LongArgs g;
    g.a = a;
    g.ids = (const uint32_t *)(base + o_ids);
    g.k = (uint32_t)k;
    g.mbase = (const uint32_t *)(base + o_mbase);
    g.wbase = (const uint32_t *)(base + o_wbase);
    g.m_read = (uint32_t *)(base + o_mread);
    g.w_read = (uint32_t *)(base + o_wread);
    g.n_mean = (uint32_t)n_mean;
    g.n_win = (uint32_t)n_win;
    g.csum = (double *)(base + o_csum);
    g.cstart = (double *)(base + o_cstart);
    g.chead = (double *)(base + o_chead);
    g.clean = (unsigned char *)(base + o_clean);
    g.mmeta = (MeanMeta *)(base + o_mmeta);
    g.wmeta = (WinMeta *)(base + o_wmeta);
    unsigned long long *tmp = (unsigned long long *)(base + o_tmp);
    hipStream_t st = ctx->stream;

    {
        flx_time_scope ts(ctx, "flx_score_phred_long");
        hipLaunchKernelGGL(flx_score_phred_long_count, dim3(G), dim3(256), 0, st, a.lengths, a.order, n, per, (int)thr,
                           (uint32_t *)(base + o_blk));
        hipLaunchKernelGGL(flx_score_phred_long_compact, dim3(G), dim3(256), 0, st, a.lengths, a.order, n, per, (int)thr,
                           (const uint32_t *)(base + o_blk), (uint32_t *)(base + o_ids));
        hipLaunchKernelGGL(flx_score_phred_long_index, dim3(1), dim3(1024), 0, st, a, g.ids, g.k, tmp, (uint32_t *)g.mbase,
                           (uint32_t *)g.wbase);
        const unsigned per_read_blocks = (unsigned)std::min<uint64_t>((k + 3) / 4, 4096);
        hipLaunchKernelGGL(flx_score_phred_long_expand, dim3(per_read_blocks), dim3(256), 0, st, g);
        hipLaunchKernelGGL(flx_score_phred_long_sums, dim3((unsigned)((n_mean + 3) / 4)), dim3(256), 0, st, g);
        hipLaunchKernelGGL(flx_score_phred_long_prefix, dim3((unsigned)k), dim3(64), 0, st, g);
        hipLaunchKernelGGL(flx_score_phred_long_maps, dim3((unsigned)((n_mean + n_win + 3) / 4)), dim3(256), 0, st, g);
        hipLaunchKernelGGL(flx_score_phred_long_walk, dim3((unsigned)k), dim3(64), 0, st, g);
        FLX_HIP(ctx, hipGetLastError());
    }
    if (report) {
        FLX_HIP(ctx, hipStreamSynchronize(st));
        const double t = std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
        fprintf(stderr, "[flx_score_batch] %-22s %8.3f ms  (%llu reads of >= %lld bases, %llu + %llu chunks)\n", "phred long reads",
                (t - t_start) * 1e3, k, thr, n_mean, n_win);
    }
    if (k == n) ctx->last_phred_kernel = "flx_score_phred_long";  // the batch kernel skipped every read
    *scored = true;
    return FLX_OK;
}
