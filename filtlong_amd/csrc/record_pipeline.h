// record_pipeline.h — the record-layout pass of bam.hip (BAM records -> FASTQ text) and bam_encode.hip (record text -> BAM records).
//
// k_sizes        one thread per record: what the codec says the record contributes, and whether it is bad; the tile's sums;
// k_scan_tiles   one workgroup: exclusive scan of the tiles' sums, the totals and the lowest bad record;
// k_offsets      the scan inside each tile: out_off[k], item_off[k], and the record of every emit item;
// the codec's emit kernel, one workgroup per (record, chunk of CHUNK bases), grid-stride over the items.
// A codec is a small struct of device pointers, passed to the kernels by value:
//   using Sums                       Sum2 (bytes, items) or Sum3 (bytes, items, skipped records);
//   static extra_bytes(n_rec)        bytes of the work block that are the codec's own (Work::extra);
//   measure(k, &bad)                 the sums of record k in the sizes pass, zero and bad for a record that is not valid
//                                    (it may keep what it found in its own array for the passes behind);
//   recall(k)                        the same sums again in the offsets pass.
#pragma once
#include "flx_internal.h"

namespace recpipe {

constexpr int NT = 256;              // threads per workgroup, records per tile
constexpr uint32_t CHUNK = 16 * NT;  // bases per emit item: one 16-byte store per lane
constexpr unsigned kEmitBlocksPerCU = 8;
// the call's state on the device (zeroed before the launches): [0] output bytes, [1] emit items, [2] skipped records (Sum3),
// [3] n_records - the lowest bad record (0: none; an atomicMax over the bad records)
constexpr int kStateWords = 4;

struct Sum2 {
    unsigned long long bytes, items;
};
struct Sum3 {
    unsigned long long bytes, items, skipped;
};
__device__ __forceinline__ Sum2 add(Sum2 a, Sum2 b) { return {a.bytes + b.bytes, a.items + b.items}; }
__device__ __forceinline__ Sum3 add(Sum3 a, Sum3 b) { return {a.bytes + b.bytes, a.items + b.items, a.skipped + b.skipped}; }
__device__ __forceinline__ Sum2 sub(Sum2 a, Sum2 b) { return {a.bytes - b.bytes, a.items - b.items}; }
__device__ __forceinline__ Sum3 sub(Sum3 a, Sum3 b) { return {a.bytes - b.bytes, a.items - b.items, a.skipped - b.skipped}; }
__device__ __forceinline__ void store_totals(unsigned long long *state, Sum2 s) { state[0] = s.bytes, state[1] = s.items; }
__device__ __forceinline__ void store_totals(unsigned long long *state, Sum3 s) { state[0] = s.bytes, state[1] = s.items, state[2] = s.skipped; }

// exclusive scan of one value per thread over the workgroup; *total gets the sum (every thread)
template <class S>
__device__ __forceinline__ S block_excl_scan(S v, S *total) {
    __shared__ S buf[2][NT];
    const int t = threadIdx.x;
    int cur = 0;
    buf[0][t] = v;
    __syncthreads();
    for (int d = 1; d < NT; d <<= 1) {
        S x = buf[cur][t];
        if (t >= d) x = add(x, buf[cur][t - d]);
        buf[cur ^ 1][t] = x;
        cur ^= 1;
        __syncthreads();
    }
    const S incl = buf[cur][t];
    *total = buf[cur][NT - 1];
    __syncthreads();  // (the next call writes buf[0])
    return sub(incl, v);
}

template <class C>
__global__ void __launch_bounds__(NT) k_sizes(C codec, uint64_t n_rec, typename C::Sums *tile_sums, unsigned long long *state) {
    const uint64_t k = (uint64_t)blockIdx.x * NT + threadIdx.x;
    typename C::Sums v = {}, total;
    if (k < n_rec) {
        bool bad;
        v = codec.measure(k, &bad);
        if (bad) atomicMax(&state[3], (unsigned long long)(n_rec - k));
    }
    block_excl_scan(v, &total);
    if (threadIdx.x == 0) tile_sums[blockIdx.x] = total;
}

template <class S>
__global__ void __launch_bounds__(NT) k_scan_tiles(S *tile_sums, uint64_t n_tiles, unsigned long long *state) {
    S carry = {};
    for (uint64_t base = 0; base < n_tiles; base += NT) {
        const uint64_t i = base + threadIdx.x;
        const S v = i < n_tiles ? tile_sums[i] : S{};
        S total;
        const S ex = block_excl_scan(v, &total);
        if (i < n_tiles) tile_sums[i] = add(carry, ex);
        carry = add(carry, total);
    }
    if (threadIdx.x == 0) store_totals(state, carry);
}

template <class C>
__global__ void __launch_bounds__(NT) k_offsets(C codec, uint64_t n_rec, const typename C::Sums *tile_sums, const unsigned long long *state,
                                                uint64_t *out_off, uint64_t *item_off, uint32_t *item_rec, uint64_t item_cap) {
    const uint64_t k = (uint64_t)blockIdx.x * NT + threadIdx.x;
    typename C::Sums v = {}, total;
    if (k < n_rec) v = codec.recall(k);
    const typename C::Sums ex = add(tile_sums[blockIdx.x], block_excl_scan(v, &total));
    if (k >= n_rec) return;
    out_off[k] = ex.bytes;
    item_off[k] = ex.items;
    if (k == n_rec - 1) {
        out_off[n_rec] = state[0];
        item_off[n_rec] = state[1];
    }
    // (item_cap is the host's bound of the item count, n_rec + bytes / CHUNK: records whose ranges do not overlap cannot exceed
    // it, and the test keeps any others from writing outside the array)
    for (uint64_t c = 0; c < v.items && ex.items + c < item_cap; ++c) item_rec[ex.items + c] = (uint32_t)k;
}

// An unaligned destination of n bytes: head bytes up to the next 16-byte boundary, whole aligned 16-byte groups, tail bytes.
struct Split16 {
    uint32_t head, groups, tail;
};
__device__ __forceinline__ Split16 split16(const uint8_t *dst, uint32_t n) {
    uint32_t head = (uint32_t)(-(uintptr_t)dst & 15);
    if (head > n) head = n;
    const uint32_t groups = (n - head) / 16;
    return {head, groups, n - head - 16 * groups};
}

// ---- host side: the work block of one call and its launches ------------------------------------------------------------------
inline uint64_t item_bound(uint64_t n_rec, uint64_t bytes) { return n_rec + bytes / CHUNK; }
inline uint64_t n_tiles_of(uint64_t n_rec) { return (n_rec + NT - 1) / NT; }
inline unsigned emit_blocks_of(const flx_ctx *ctx) {
    return (unsigned)(ctx->prop.multiProcessorCount > 0 ? ctx->prop.multiProcessorCount : 256) * kEmitBlocksPerCU;
}

template <class C>
struct Work {  // the device arrays of one call, carved out of one block
    typename C::Sums *tile_sums;
    unsigned long long *state;
    uint64_t *item_off;
    void *extra;
    uint32_t *item_rec;
    uint64_t item_cap;
};
template <class C>
size_t work_bytes(uint64_t n_rec, uint64_t bytes) {
    return (size_t)(n_tiles_of(n_rec) * sizeof(typename C::Sums) + kStateWords * 8 + (n_rec + 1) * 8 + C::extra_bytes(n_rec) +
                    item_bound(n_rec, bytes) * 4 + 64);
}
template <class C>
Work<C> carve(void *p, uint64_t n_rec, uint64_t bytes) {
    Work<C> w;
    uint8_t *b = (uint8_t *)p;
    w.tile_sums = (typename C::Sums *)b;
    b += n_tiles_of(n_rec) * sizeof(typename C::Sums);
    w.state = (unsigned long long *)b;
    b += kStateWords * 8;
    w.item_off = (uint64_t *)b;
    b += (n_rec + 1) * 8;
    w.extra = b;
    b += C::extra_bytes(n_rec);
    w.item_rec = (uint32_t *)b;
    w.item_cap = item_bound(n_rec, bytes);
    return w;
}

template <class C>
using EmitKernel = void (*)(C codec, uint64_t n_rec, const uint64_t *out_off, const uint64_t *item_off, const uint32_t *item_rec,
                            uint64_t item_cap, unsigned long long *state, uint8_t *out, uint64_t out_cap);

// The launches of one call on `st` (n_rec >= 1): h_state (pinned, or read after a synchronisation) gets the state words.
// d_out_off may be an array of the work block.
template <class C>
hipError_t launch(hipStream_t st, unsigned emit_blocks, const C &codec, uint64_t n_rec, const Work<C> &w, uint64_t *d_out_off,
                  EmitKernel<C> emit, void *d_out, uint64_t out_cap, uint64_t *h_state) {
    hipError_t e = hipMemsetAsync(w.state, 0, kStateWords * 8, st);
    if (e != hipSuccess) return e;
    const uint64_t tiles = n_tiles_of(n_rec);
    hipLaunchKernelGGL(k_sizes<C>, dim3((unsigned)tiles), dim3(NT), 0, st, codec, n_rec, w.tile_sums, w.state);
    hipLaunchKernelGGL(k_scan_tiles<typename C::Sums>, dim3(1), dim3(NT), 0, st, w.tile_sums, tiles, w.state);
    hipLaunchKernelGGL(k_offsets<C>, dim3((unsigned)tiles), dim3(NT), 0, st, codec, n_rec, w.tile_sums, w.state, d_out_off, w.item_off,
                       w.item_rec, w.item_cap);
    const uint64_t blocks = w.item_cap < emit_blocks ? w.item_cap : emit_blocks;
    hipLaunchKernelGGL(emit, dim3((unsigned)(blocks ? blocks : 1)), dim3(NT), 0, st, codec, n_rec, d_out_off, w.item_off, w.item_rec,
                       w.item_cap, w.state, (uint8_t *)d_out, out_cap);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    return hipMemcpyAsync(h_state, w.state, kStateWords * 8, hipMemcpyDeviceToHost, st);
}

inline uint64_t first_bad_of(const uint64_t *st, uint64_t n_rec) { return n_rec - (st[3] <= n_rec ? st[3] : n_rec); }

// The tail of a device-resident entry point `fn`: waits for the stream behind launch(), then *first_bad, *out_len and the
// capacity error from the state words.
inline int finish_dev(flx_ctx *ctx, const char *fn, hipError_t e, const uint64_t *st, uint64_t n_rec, uint64_t out_cap, uint64_t *out_len,
                      uint64_t *first_bad) {
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return flx_fail(ctx, FLX_ERR_HIP, "%s: %s", fn, hipGetErrorString(e));
    *first_bad = first_bad_of(st, n_rec);
    *out_len = st[0];
    if (st[0] > out_cap)
        return flx_fail(ctx, FLX_ERR_CAPACITY, "%s: %llu bytes needed, capacity %llu", fn, (unsigned long long)st[0], (unsigned long long)out_cap);
    return FLX_OK;
}

}  // namespace recpipe
