// qsplit.hip — --split_window_q on the GPU: reads split at low-quality windows in Phred mode (the definition: qsplit.h).
//
//   detection     one wave per read, 1024 bases a step: lane l takes the 16 bases from p0 + 16 l with one aligned 16-byte load.  Two
//                 running prefix sums of E, W bases apart, give every window's sum: the leading edge at base j and the trailing edge
//                 at j - n, both out of the plane (the second comes out of L2; any window size, no history ring).  Only their
//                 difference matters, so it is one scan: lane-local sums of both edges, a wave scan of (leading - trailing) per lane
//                 and a uint64 carry from step to step; the next step's 32 bytes are requested before this step's are used.  The
//                 1 KiB table of E sits in LDS.  A max-scan of "the last bad end so far" gives every bad end its predecessor, which is
//                 all the child rule needs; a step without a bad window (a wave-uniform test) skips that part.
//                 The kernel runs twice: a count pass (children per read, first / last), an exclusive scan into child_offsets, and
//                 an emit pass that writes the ranges and the parents and leaves a read without children at once.
//   child plane   the children's bytes gathered into a plane of their own by flx_plane_layout's rule (16-byte slots, 128-byte
//                 starts from 1024 bases on): a slot scan, then one wave per child, whole 16-byte stores to aligned slots from loads at
//                 whatever address the child starts (the hardware's unaligned global loads), the last slot's tail zero.
//   scoring       flx_launch_score_phred over the child plane, children by descending length: a child's scores are the bits
//                 flx_score_batch gives its quality substring, long children take the cooperative path by themselves.
#include <algorithm>

#include "flx_internal.h"
#include "qsplit.h"
#include "rank_internal.h"

namespace {

__constant__ uint32_t c_error_table[256] = {QSPLIT_ERROR_TABLE};

constexpr int kLaneBases = 16;                // bases per lane and step: one 16-byte load
constexpr int kStepBases = 64 * kLaneBases;   // bases per wave and step
constexpr int kWaves = 4;                     // reads per workgroup

struct DetectArgs {
    const uint8_t *plane;
    const uint64_t *offsets;
    const int32_t *lengths;
    uint64_t n_reads;
    int64_t w;        // --window_size
    uint64_t t;       // the threshold per base
    // count pass
    int64_t *n_child;  // [n_reads]
    int32_t *first, *last;
    // emit pass
    const uint64_t *child_offsets;
    int32_t *child_ranges;
    uint32_t *child_parent;
    uint64_t capacity;
};

__device__ __forceinline__ uint64_t wave_scan_add(uint64_t v, int lane) {  // inclusive
    for (int o = 1; o < 64; o <<= 1) {
        const uint64_t u = __shfl_up((unsigned long long)v, (unsigned)o, 64);
        if (lane >= o) v += u;
    }
    return v;
}
__device__ __forceinline__ uint32_t wave_scan_add(uint32_t v, int lane) {
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t u = __shfl_up(v, (unsigned)o, 64);
        if (lane >= o) v += u;
    }
    return v;
}
__device__ __forceinline__ int32_t wave_scan_max(int32_t v, int lane) {
    for (int o = 1; o < 64; o <<= 1) {
        const int32_t u = __shfl_up(v, (unsigned)o, 64);
        if (lane >= o) v = max(v, u);
    }
    return v;
}

// The 16 bytes q[at, at + 16) of a read of l bases whose slot holds lpad = round_up(l, 16) bytes; bytes outside [0, l) come back as
// whatever (the caller masks them by index) but are never read outside [0, lpad).
__device__ __forceinline__ void load16(const uint8_t *q, int64_t at, int64_t l, int64_t lpad, uint8_t b[16]) {
    if (at >= 0 && at + 16 <= lpad) {
        __builtin_memcpy(b, q + at, 16);  // (any alignment)
    } else {
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const int64_t i = at + k;
            b[k] = i >= 0 && i < l ? q[i] : 0;
        }
    }
}

template <bool EMIT>
__global__ void __launch_bounds__(kWaves * 64) k_qsplit_detect(const DetectArgs a) {
    __shared__ uint32_t tab[256];
    tab[threadIdx.x] = c_error_table[threadIdx.x];
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const uint64_t r = (uint64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (r >= a.n_reads) return;
    const int64_t l = a.lengths[r];
    if (l <= 0) {
        if (!EMIT && lane == 0) {
            a.n_child[r] = 0;
            a.first[r] = 0;
            a.last[r] = 0;
        }
        return;
    }
    const uint8_t *q = a.plane + a.offsets[r];
    const int64_t lpad = (l + 15) & ~(int64_t)15;
    const int64_t n = a.w < l ? a.w : l;
    const uint64_t limit = a.t * (uint64_t)n;
    const uint64_t out_base = EMIT ? a.child_offsets[r] : 0;

    if (EMIT && a.child_offsets[r + 1] == out_base) return;  // (the count pass found no child: nothing to write)

    uint64_t carry = 0;                        // sum of E over [p0 + 1 - n, p0): the leading sum over [0, p0) minus the trailing one
    int32_t prev_carry = -1;                   // the last bad end in front of this step
    uint64_t n_out = 0;                        // children so far
    int32_t my_first = 0x7fffffff, my_last = -1;

    auto emit = [&](uint64_t k, int32_t s, int32_t e) {
        my_first = min(my_first, s);
        my_last = max(my_last, e);
        if (EMIT) {
            const uint64_t at = out_base + k;
            if (at < a.capacity) {
                a.child_ranges[2 * at] = s;
                a.child_ranges[2 * at + 1] = e;
                a.child_parent[at] = (uint32_t)r;
            }
        }
    };

    // the 16 leading and the 16 trailing bytes of this lane for the step at p0 (bytes outside the read: whatever, masked by index)
    auto fetch = [&](int64_t p0, uint4 &lv, uint4 &tv) {
        const int64_t pos = p0 + (int64_t)lane * kLaneBases, tpos = pos + 1 - n;
        lv = make_uint4(0, 0, 0, 0);
        tv = make_uint4(0, 0, 0, 0);
        if (pos < lpad) lv = *(const uint4 *)(q + pos);  // (16-byte aligned: the plane's rule)
        if (tpos + 16 > 0 && tpos < l) load16(q, tpos, l, lpad, (uint8_t *)&tv);
    };
    uint4 lnext, tnext;
    fetch(0, lnext, tnext);
    for (int64_t p0 = 0; p0 < l; p0 += kStepBases) {
        const int64_t pos = p0 + (int64_t)lane * kLaneBases;  // this lane's first leading base = its first window end
        const int64_t tpos = pos + 1 - n;                      // ... and its first trailing position
        alignas(16) uint8_t lb[16], tb[16];
        *(uint4 *)lb = lnext;
        *(uint4 *)tb = tnext;
        if (p0 + kStepBases < l) fetch(p0 + kStepBases, lnext, tnext);  // (the next step's bytes are on their way during this one)
        uint32_t le[16], te[16];
        uint64_t lsum = 0, tsum = 0;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            le[k] = pos + k < l ? tab[lb[k]] : 0u;
            te[k] = tpos + k >= 0 && tpos + k < l ? tab[tb[k]] : 0u;
            lsum += le[k];
            tsum += te[k];
        }
        // ONE scan, of leading minus trailing (modulo 2^64: every true window sum is non-negative and below 2^63)
        const uint64_t d = lsum - tsum, dscan = wave_scan_add(d, lane);
        uint64_t win = carry + (dscan - d);  // sum of E over [tpos, pos)
        carry += __shfl((unsigned long long)dscan, 63, 64);
        uint32_t bad = 0;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            win += le[k];  // ... over [j - n + 1, j], j = pos + k
            const int64_t j = pos + k;
            if (j >= n - 1 && j < l && win > limit) bad |= 1u << k;
            win -= te[k];
        }
        if (__ballot(bad != 0) == 0) continue;  // (wave-uniform)

        const int32_t lane_last = bad ? (int32_t)(pos + (31 - __clz((int)bad))) : -1;
        const int32_t last_scan = wave_scan_max(lane_last, lane);
        int32_t before = __shfl_up(last_scan, 1u, 64);
        before = lane ? max(before, prev_carry) : prev_carry;
        prev_carry = max(prev_carry, __shfl(last_scan, 63, 64));
        // this lane's children: one in front of a bad end whose predecessor lies more than W back (or that has none)
        uint32_t cnt = 0;
        {
            int64_t prev = before;
            for (uint32_t m = bad; m; m &= m - 1) {
                const int64_t j = pos + (__ffs((int)m) - 1);
                int32_t s, e;
                cnt += qsplit::child_before(prev, j, n, a.w, &s, &e) ? 1u : 0u;
                prev = j;
            }
        }
        const uint32_t cscan = wave_scan_add(cnt, lane);
        if (cnt) {
            uint64_t k = n_out + (cscan - cnt);
            int64_t prev = before;
            for (uint32_t m = bad; m; m &= m - 1) {
                const int64_t j = pos + (__ffs((int)m) - 1);
                int32_t s, e;
                if (qsplit::child_before(prev, j, n, a.w, &s, &e)) emit(k++, s, e);
                prev = j;
            }
        }
        n_out += __shfl(cscan, 63, 64);
    }

    // the trailing child, and the read's summary
    const bool any_bad = prev_carry >= 0;
    if (any_bad && (int64_t)prev_carry + 1 < l) {
        if (lane == 0) emit(n_out, prev_carry + 1, (int32_t)l);
        ++n_out;
    }
    if (!EMIT) {
        for (int o = 32; o; o >>= 1) {
            my_first = min(my_first, __shfl_xor(my_first, o, 64));
            my_last = max(my_last, __shfl_xor(my_last, o, 64));
        }
        if (lane == 0) {
            a.n_child[r] = (int64_t)n_out;
            a.first[r] = !any_bad ? 0 : n_out ? my_first : -1;
            a.last[r] = !any_bad ? (int32_t)l : n_out ? my_last : -1;
        }
    }
}

// a read with bad windows and no child fails (after the parents' scoring has written its flag)
__global__ void __launch_bounds__(256) k_qsplit_fail_wholly_bad(uint64_t n, const int32_t *first, const int32_t *lengths, uint8_t *passed) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n && first[i] < 0 && lengths[i] > 0) passed[i] = 0;
}

// per child: its length, its slot in the child plane (16-byte slots; a child of 1024 bases or more gets room to start on a 128-byte
// line wherever the scan puts it) and its sort key (descending length)
__global__ void __launch_bounds__(256) k_qsplit_child_slots(uint64_t nc, const int32_t *ranges, int32_t *len, int64_t *slot, uint64_t *key, uint32_t *val) {
    const uint64_t c = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (c > nc) return;
    if (c == nc) {
        slot[c] = 0;  // (the scan's last entry is the total)
        return;
    }
    const int32_t cl = ranges[2 * c + 1] - ranges[2 * c];
    len[c] = cl;
    slot[c] = (((int64_t)cl + 15) & ~(int64_t)15) + (cl >= 1024 ? 112 : 0);
    key[c] = (uint64_t)(0x7fffffff - cl);
    val[c] = (uint32_t)c;
}

__global__ void __launch_bounds__(256) k_qsplit_child_starts(uint64_t nc, const int32_t *len, uint64_t *off) {
    const uint64_t c = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (c < nc && len[c] >= 1024) off[c] = (off[c] + 127) & ~(uint64_t)127;
}

// one wave per child: 16-byte stores to the child's aligned slots, loads at whatever address the child starts in its parent
__global__ void __launch_bounds__(256) k_qsplit_gather(uint64_t nc, const uint8_t *plane, const uint64_t *offsets, const int32_t *lengths,
                                                       const int32_t *ranges, const uint32_t *parent, const uint64_t *child_off, uint8_t *child_plane) {
    const int lane = threadIdx.x & 63;
    const uint64_t c = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c >= nc) return;
    const uint32_t r = parent[c];
    const int64_t start = ranges[2 * c], cl = ranges[2 * c + 1] - start;
    const int64_t l = lengths[r], lpad = (l + 15) & ~(int64_t)15;
    const uint8_t *q = plane + offsets[r];
    uint8_t *out = child_plane + child_off[c];
    for (int64_t at = (int64_t)lane * 16; at < cl; at += 64 * 16) {
        alignas(16) uint8_t b[16];
        load16(q, start + at, l, lpad, b);
#pragma unroll
        for (int k = 0; k < 16; ++k)
            if (at + k >= cl) b[k] = 0;  // (the slot's tail)
        *(uint4 *)(out + at) = *(const uint4 *)b;
    }
}

int validate(flx_ctx *ctx, uint64_t n_reads, uint64_t plane_bytes, const flx_params *params, double split_window_q, const flx_scores *out,
             uint64_t *t) {
    if (!ctx) return FLX_ERR_INVALID;
    if (!params || !out) return flx_fail(ctx, FLX_ERR_INVALID, "params/out must not be NULL");
    if (n_reads > 0xffffffffull) return flx_fail(ctx, FLX_ERR_INVALID, "at most 2^32-1 reads per batch");
    if (plane_bytes & 15) return flx_fail(ctx, FLX_ERR_INVALID, "plane_bytes must be a multiple of 16");
    if (n_reads && (!out->mean_q || !out->window_q || !out->passed))
        return flx_fail(ctx, FLX_ERR_INVALID, "mean_q/window_q/passed outputs are required");
    if (params->window_size <= 0) return flx_fail(ctx, FLX_ERR_INVALID, "window_size must be positive");
    if (params->trim || params->split_set) return flx_fail(ctx, FLX_ERR_INVALID, "trim/split need a k-mer set: not with split_window_q");
    if (!out->child_offsets) return flx_fail(ctx, FLX_ERR_INVALID, "split_window_q requested but child_offsets is NULL");
    if (!qsplit::threshold(split_window_q, t)) return flx_fail(ctx, FLX_ERR_INVALID, "split_window_q must be greater than 0 and less than 100");
    return FLX_OK;
}

}  // namespace

extern "C" int flx_qsplit_table(uint32_t e[256]) {
    if (!e) return FLX_ERR_INVALID;
    memcpy(e, qsplit::kErrorTable, sizeof qsplit::kErrorTable);
    return FLX_OK;
}

extern "C" int flx_qsplit_threshold(double q, uint64_t *t) {
    return t && qsplit::threshold(q, t) ? FLX_OK : FLX_ERR_INVALID;
}

extern "C" int flx_score_batch_qsplit_dev(flx_ctx *ctx, const void *d_plane, uint64_t plane_bytes, const void *d_offsets, const void *d_lengths,
                                          const void *d_order, uint64_t n_reads, const flx_params *params, double split_window_q,
                                          flx_scores *out) {
    uint64_t t = 0;
    FLX_CHECK(validate(ctx, n_reads, plane_bytes, params, split_window_q, out, &t));
    out->n_children = 0;
    if (n_reads == 0) return FLX_OK;
    FLX_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
    char *wp = nullptr;
    auto carve = [&](size_t bytes) { void *p = wp; wp += up(bytes); return p; };

    // ---- per-read arrays (workspace 0) ----
    const size_t scan_ws = flx_radix_sort_workspace(n_reads + 1);
    void *small = nullptr;
    FLX_CHECK(flx_workspace(ctx, 0, up((n_reads + 1) * 8) + 2 * up(n_reads * 4) + up(scan_ws), &small));
    wp = (char *)small;
    int64_t *d_nchild = (int64_t *)carve((n_reads + 1) * 8);
    int32_t *d_first_tmp = (int32_t *)carve(n_reads * 4), *d_last_tmp = (int32_t *)carve(n_reads * 4);
    void *d_scanws = carve(scan_ws);
    int32_t *first = out->first ? out->first : d_first_tmp, *last = out->last ? out->last : d_last_tmp;

    DetectArgs a;
    memset(&a, 0, sizeof a);
    a.plane = (const uint8_t *)d_plane;
    a.offsets = (const uint64_t *)d_offsets;
    a.lengths = (const int32_t *)d_lengths;
    a.n_reads = n_reads;
    a.w = params->window_size;
    a.t = t;
    a.n_child = d_nchild;
    a.first = first;
    a.last = last;
    const unsigned grid = (unsigned)((n_reads + kWaves - 1) / kWaves);

    // ---- count pass -> child_offsets ----
    FLX_HIP(ctx, hipMemsetAsync(d_nchild + n_reads, 0, 8, st));
    {
        flx_time_scope ti(ctx, "flx_qsplit_detect.count");
        hipLaunchKernelGGL(k_qsplit_detect<false>, dim3(grid), dim3(kWaves * 64), 0, st, a);
    }
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

    a.child_offsets = out->child_offsets;
    a.child_ranges = out->child_ranges;
    a.capacity = nc;
    return flx_phred_children(ctx, d_plane, plane_bytes, d_offsets, d_lengths, d_order, n_reads, params, out, first, nc, [&](uint32_t *d_parent) {
        a.child_parent = d_parent;
        flx_time_scope ti(ctx, "flx_qsplit_detect.emit");
        hipLaunchKernelGGL(k_qsplit_detect<true>, dim3(grid), dim3(kWaves * 64), 0, st, a);
        ti.end();
        FLX_HIP(ctx, hipGetLastError());
        return (int)FLX_OK;
    });
}

// What a Phred-mode call with children does once the producer of the children has filled first / last and out->child_offsets and knows
// their number: the parents' scoring, the producer's emit pass (child_ranges and the parent of every child), then the child plane and
// the children's scoring.  Shared by --split_window_q above and --trim_adapters (adapters.hip).
int flx_phred_children(flx_ctx *ctx, const void *d_plane, uint64_t plane_bytes, const void *d_offsets, const void *d_lengths, const void *d_order,
                       uint64_t n_reads, const flx_params *params, flx_scores *out, const int32_t *first, uint64_t nc,
                       const std::function<int(uint32_t *d_parent)> &emit) {
    hipStream_t st = ctx->stream;
    auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
    char *wp = nullptr;
    auto carve = [&](size_t bytes) { void *p = wp; wp += up(bytes); return p; };

    // ---- the parents: today's scoring, untouched; a read with no base left fails ----
    flx_score_out_dev po{out->mean_q, out->window_q, out->passed};
    FLX_CHECK(flx_launch_score_phred(ctx, (const uint8_t *)d_plane, plane_bytes, (const uint64_t *)d_offsets, (const int32_t *)d_lengths,
                                     (const uint32_t *)d_order, n_reads, params, po));
    if (nc == 0) {
        FLX_HIP(ctx, hipStreamSynchronize(st));
        FLX_CHECK(flx_phred_finish(ctx));
        hipLaunchKernelGGL(k_qsplit_fail_wholly_bad, dim3((unsigned)((n_reads + 255) / 256)), dim3(256), 0, st, n_reads, first, (const int32_t *)d_lengths, out->passed);
        FLX_HIP(ctx, hipGetLastError());
        FLX_HIP(ctx, hipStreamSynchronize(st));
        return FLX_OK;
    }

    // ---- emit pass, the children's slots and order (workspace 2) ----
    const size_t sort_ws = flx_radix_sort_workspace(nc + 1);
    void *cw = nullptr;
    FLX_CHECK(flx_workspace(ctx, 2, 3 * up((nc + 1) * 8) + 4 * up(nc * 4) + 2 * up(nc * 8) + up(sort_ws), &cw));
    wp = (char *)cw;
    int64_t *d_slot = (int64_t *)carve((nc + 1) * 8);
    uint64_t *d_coff = (uint64_t *)carve((nc + 1) * 8);
    uint64_t *keys0 = (uint64_t *)carve(nc * 8), *keys1 = (uint64_t *)carve(nc * 8);
    uint32_t *vals0 = (uint32_t *)carve(nc * 4), *vals1 = (uint32_t *)carve(nc * 4);
    uint32_t *d_parent = (uint32_t *)carve(nc * 4);
    int32_t *d_clen = (int32_t *)carve(nc * 4);
    void *d_sortws = carve(sort_ws);
    FLX_CHECK(emit(d_parent));
    const unsigned cgrid = (unsigned)((nc + 1 + 255) / 256);
    uint64_t child_plane_bytes = 0;
    uint64_t *skeys = nullptr;
    uint32_t *d_corder = nullptr;
    {
        flx_time_scope ti(ctx, "flx_qsplit_children.layout");
        hipLaunchKernelGGL(k_qsplit_child_slots, dim3(cgrid), dim3(256), 0, st, nc, (const int32_t *)out->child_ranges, d_clen, d_slot, keys0, vals0);
        FLX_HIP(ctx, hipGetLastError());
        FLX_CHECK(flx_exclusive_scan_i64(ctx, nc + 1, d_slot, (int64_t *)d_coff, d_sortws, sort_ws));
        FLX_HIP(ctx, hipMemcpyAsync(&child_plane_bytes, d_coff + nc, 8, hipMemcpyDeviceToHost, st));
        hipLaunchKernelGGL(k_qsplit_child_starts, dim3(cgrid), dim3(256), 0, st, nc, (const int32_t *)d_clen, d_coff);
        FLX_HIP(ctx, hipGetLastError());
        FLX_CHECK(flx_radix_sort_pairs(ctx, nc, keys0, keys1, vals0, vals1, d_sortws, sort_ws, &skeys, &d_corder));
    }
    // (this wait also ends the parents' call: its long reads are scored before the children's call takes the context's one pending record)
    FLX_HIP(ctx, hipStreamSynchronize(st));
    FLX_CHECK(flx_phred_finish(ctx));
    hipLaunchKernelGGL(k_qsplit_fail_wholly_bad, dim3((unsigned)((n_reads + 255) / 256)), dim3(256), 0, st, n_reads, first, (const int32_t *)d_lengths, out->passed);
    FLX_HIP(ctx, hipGetLastError());

    // ---- the child plane (workspace 1): slots of whole 16 bytes, the gaps in front of 128-byte starts zero ----
    child_plane_bytes = (child_plane_bytes + 15) & ~15ull;
    void *d_cplane = nullptr;
    FLX_CHECK(flx_workspace(ctx, 1, child_plane_bytes + 256, &d_cplane));
    {
        flx_time_scope ti(ctx, "flx_qsplit_children.gather");
        FLX_HIP(ctx, hipMemsetAsync(d_cplane, 0, child_plane_bytes + 256, st));
        hipLaunchKernelGGL(k_qsplit_gather, dim3((unsigned)((nc + 3) / 4)), dim3(256), 0, st, nc, (const uint8_t *)d_plane, (const uint64_t *)d_offsets,
                           (const int32_t *)d_lengths, (const int32_t *)out->child_ranges, (const uint32_t *)d_parent, (const uint64_t *)d_coff, (uint8_t *)d_cplane);
    }
    FLX_HIP(ctx, hipGetLastError());

    // ---- the children's scores: each child as a read of its own ----
    flx_score_out_dev co{out->child_mean_q, out->child_window_q, out->child_passed};
    FLX_CHECK(flx_launch_score_phred(ctx, (const uint8_t *)d_cplane, child_plane_bytes, d_coff, d_clen, d_corder, nc, params, co));
    FLX_HIP(ctx, hipStreamSynchronize(st));
    return flx_phred_finish(ctx);
}
