// bgzf_inflate.hip — BGZF members inflated on the GPU: the read side of bgzf.hip.
//
// flx_bgzf_index        (host) the well-formed BGZF members at the front of a buffer: their offsets and the offsets of their bytes;
// k_bgzf_inflate        one wave per member (the phases of bgzf_inflate_member.h): the member's bytes and its status word;
// k_bgzf_first_bad      one workgroup: the lowest member whose status is not 0.
// A BGZF member depends on no other, so the parallelism is across members; inside a member lane 0 decodes and all 64 lanes copy.
// The member's output sits in LDS (75,656 bytes = 73.9 KiB with the tables: two members per CU), so a match never reads global
// memory and nothing reaches the output buffer before the member's CRC-32 has been checked.
#include "flx_internal.h"
#include "bgzf_inflate_member.h"
#include "gzip_framing.h"

using namespace bgzf_inf;

namespace {

constexpr int kFirstBadThreads = 256;

__global__ void __launch_bounds__(BI_NT) k_bgzf_inflate(const uint8_t *in, const uint64_t *in_off, const uint64_t *out_off,
                                                        uint8_t *out, uint32_t *status) {
    __shared__ Shared S;
    const int t = threadIdx.x;
    const uint64_t k = blockIdx.x;
    const uint64_t at = in_off[k], end = in_off[k + 1];
    const uint64_t o0 = out_off[k], o1 = out_off[k + 1];
    const uint8_t *m = in + at;
    // (a member of more than 64 KiB is refused by ph_init before it reads a byte)
    const uint32_t msize = end > at && end - at <= 65536 ? (uint32_t)(end - at) : 0;
    ph_init(t, S, m, msize, o1 >= o0 ? o1 - o0 : ~0ull);
    __syncthreads();
    const uint32_t cap = max_rounds(S);
    for (uint32_t r = 0; S.mode != M_DONE; ++r) {  // (S.mode is read behind a barrier: uniform)
        if (r >= cap) {
            __syncthreads();
            if (t == 0) fail(S, ST_ROUNDS);
            __syncthreads();
            break;
        }
        ph_window(t, S, m);
        __syncthreads();
        ph_decode(t, S);
        __syncthreads();
        ph_tables_clear(t, S);
        __syncthreads();
        ph_tables_fill(t, S);
        ph_stored(t, S, m);
        ph_literals(t, S);
        __syncthreads();
        const int nm = S.n_mat;
        for (int j = 0; j < nm; ++j) {
            ph_match(t, S, j);
            __syncthreads();
        }
    }
    ph_end(t, S);
    __syncthreads();
    ph_crc(t, S);
    __syncthreads();
    ph_crc_final(t, S);
    __syncthreads();
    ph_store(t, S, out + o0, status + k);
}

__global__ void __launch_bounds__(kFirstBadThreads) k_bgzf_first_bad(const uint32_t *status, uint64_t n, uint64_t *first_bad) {
    __shared__ unsigned long long best[kFirstBadThreads];
    unsigned long long b = n;
    for (uint64_t k = threadIdx.x; k < n; k += kFirstBadThreads)
        if (status[k] != 0 && k < b) b = k;
    best[threadIdx.x] = b;
    __syncthreads();
    for (int d = kFirstBadThreads / 2; d > 0; d >>= 1) {
        if ((int)threadIdx.x < d && best[threadIdx.x + d] < best[threadIdx.x]) best[threadIdx.x] = best[threadIdx.x + d];
        __syncthreads();
    }
    if (threadIdx.x == 0) *first_bad = best[0];
}

}  // namespace

// the two launches of one call on `st`; *d_first (device) gets the lowest bad member
hipError_t flx_bgzf_inflate_launch(hipStream_t st, const void *d_in, const uint64_t *d_in_off, const uint64_t *d_out_off,
                                   uint64_t n_members, void *d_out, uint32_t *d_status, uint64_t *d_first) {
    for (uint64_t first = 0; first < n_members; first += 1u << 30) {  // (the grid's x dimension)
        const uint32_t b = (uint32_t)(n_members - first < (1u << 30) ? n_members - first : 1u << 30);
        hipLaunchKernelGGL(k_bgzf_inflate, dim3(b), dim3(BI_NT), 0, st, (const uint8_t *)d_in, d_in_off + first, d_out_off + first,
                           (uint8_t *)d_out, d_status + first);
    }
    hipLaunchKernelGGL(k_bgzf_first_bad, dim3(1), dim3(kFirstBadThreads), 0, st, d_status, n_members, d_first);
    return hipGetLastError();
}

extern "C" int flx_bgzf_index(const void *in, uint64_t n, uint64_t max_members, uint64_t *in_off, uint64_t *out_off,
                              uint64_t *n_members) {
    if ((!in && n) || !in_off || !out_off || !n_members) return FLX_ERR_INVALID;
    const uint8_t *d = (const uint8_t *)in;
    uint64_t at = 0, out = 0, m = 0;
    in_off[0] = 0;
    out_off[0] = 0;
    gzframe::Member mem;
    while (m < max_members && gzframe::member_at(d, (size_t)n, (size_t)at, &mem) == gzframe::Kind::BGZF) {
        at += mem.size;
        out += mem.isize;
        ++m;
        in_off[m] = at;
        out_off[m] = out;
    }
    *n_members = m;
    return FLX_OK;
}

extern "C" int flx_bgzf_inflate_dev(flx_ctx *ctx, const void *d_in, const uint64_t *d_in_off, const uint64_t *d_out_off,
                                    uint64_t n_members, void *d_out, uint32_t *d_status, uint64_t *first_bad) {
    if (!ctx) return FLX_ERR_INVALID;
    if (!first_bad) return flx_fail(ctx, FLX_ERR_INVALID, "flx_bgzf_inflate_dev: bad argument");
    *first_bad = n_members;
    if (n_members == 0) return FLX_OK;
    if (!d_in || !d_in_off || !d_out_off || !d_status) return flx_fail(ctx, FLX_ERR_INVALID, "flx_bgzf_inflate_dev: bad argument");
    void *work = nullptr;
    FLX_CHECK(flx_scratch(ctx, 8, &work));
    flx_time_scope ts(ctx, "flx_bgzf_inflate");
    hipError_t e = flx_bgzf_inflate_launch(ctx->stream, d_in, d_in_off, d_out_off, n_members, d_out, d_status, (uint64_t *)work);
    ts.end();
    uint64_t fb = n_members;
    if (e == hipSuccess) e = hipMemcpyAsync(&fb, work, 8, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return flx_fail(ctx, FLX_ERR_HIP, "flx_bgzf_inflate_dev: %s", hipGetErrorString(e));
    *first_bad = fb;
    return FLX_OK;
}
