// screen_hash.hip — --exclude_k K: the contaminant screen with K-mers of 17..31 bases (16 too, for the cross-check), kept as an
// open-addressing table of 64-bit canonical keys in device memory (screen_hash.h has the definition and the table's rules).
//
// The bitmap of screen.hip is exact for 16-mers and nothing else: an unrelated read keeps |X| / 2^32 of its windows, so a genome
// cannot be screened with it.  A K-mer of up to 31 bases is a 62-bit number; the set of those of a reference is sparse in 2^62 and
// is stored by hash.  Both kernels walk their sequences the same way, the way k_screen_hits walks reads (walk_spans below): a work
// item is a SPAN of kScreenSpan window starts of one sequence, found through the segment table (screen_walk.h: span_of); a lane owns
// 16 consecutive window starts, i.e. the bytes p .. p + 14 + K <= p + 45 of three aligned 16-byte loads, and turns them into two words
// of 2-bit codes and a validity mask (lane_words, on the byte helpers of screen_walk.h); window_key cuts window j out of them.  One
// 250 Mbp chromosome is sixty thousand spans.
//
//   k_screenset_insert   every valid window's canonical key goes into the table: a 64-bit atomicCAS on the slot — empty: taken,
//                        equal: stored already, other: the next slot.  Only the lane whose CAS took an empty slot counts a new key;
//                        the counts are summed per wave and span and added with one atomicAdd.
//   k_screenset_rehash   every stored key of a table into a larger, empty one (the same CAS; keys are distinct, nothing is counted)
//   k_screen_hits_hash   persistent workgroups; wave w of the grid takes the spans w, w + waves, ...; the next step's bytes are
//                        requested before this step's are used; the first probes of eight windows are in flight together, a probe
//                        chain goes on until the key or an empty slot; one atomicAdd per wave and span into hits[read].
#include "screen_internal.h"
#include "screen_walk.h"

struct flx_screenset {
    flx_ctx *ctx = nullptr;
    int k = 0;
    uint64_t capacity = 0;      // slots, a power of two, at least twice `size` after every add
    uint64_t *d_table = nullptr;
    uint64_t *d_count = nullptr;  // the stored keys, counted by the insert kernel
    uint64_t size = 0;
    bool final = false;
    unsigned blocks = 0;  // resident workgroups of the walking kernels on this device
};

namespace {

using screen::kScreenSpan;
using screen::kScreenStep;
using screen_walk::codes16;
using screen_walk::span_of;
using screen_walk::u32x4;
using screen_walk::valid16;
using screenk::kEmpty;

constexpr int kHashThreads = 256;
constexpr int kGroup = 8;  // windows of a lane whose first probes are in flight together

// The lane's 48 bytes as codes and windows.  hi: bases 0..31, base b in bits 2 (31 - b) + 1 .. 2 (31 - b); lo: bases 32..47 in the
// upper half the same way, the lower half zero.  Returns bit j (j < 16): the K bytes from base j on are all in ACGTacgt and j < left,
// the window starts this lane has left in its span.  What both kernels know about a lane's windows comes from here and window_key.
__device__ __forceinline__ uint32_t lane_words(u32x4 a, u32x4 b, u32x4 c, int k, uint32_t left, uint64_t *hi, uint64_t *lo) {
    *hi = ((uint64_t)codes16(a) << 32) | (uint64_t)codes16(b);
    *lo = (uint64_t)codes16(c) << 32;
    const uint64_t vm = (uint64_t)valid16(a) | ((uint64_t)valid16(b) << 16) | ((uint64_t)valid16(c) << 32);
    const uint64_t all = (1ull << k) - 1ull;
    uint32_t wv = 0;
#pragma unroll
    for (int j = 0; j < 16; ++j) wv |= (((vm >> j) & all) == all ? 1u : 0u) << j;
    if (left < 16u) wv &= (1u << left) - 1u;
    return wv;
}
// the canonical key of the window that starts at the lane's base j (j < 16)
__device__ __forceinline__ uint64_t window_key(uint64_t hi, uint64_t lo, int j, int k) {
    const uint64_t top = j == 0 ? hi : ((hi << (2 * j)) | (lo >> (64 - 2 * j)));
    return screenk::canonical(top >> (64 - 2 * k), k);
}

// The walk both kernels share.  Wave `wave` of `n_waves` takes the spans wave, wave + n_waves, ... of the segment table; for every
// step of a span op.step(hi, lo, wv) returns what the lane found in its windows, and op.done(read, sum) gets the wave's sum for the
// span in lane 0.  Loads stay inside [offset, offset + round_up(L, 16)): the first is issued for p < w1 <= L - K + 1 only, the second
// and third only if their first byte is below round_up(L, 16).  A byte that is not loaded is zero, which is no base.
template <class Op>
__device__ __forceinline__ void walk_spans(const uint8_t *__restrict__ plane, const uint64_t *__restrict__ offsets, const int32_t *__restrict__ lengths,
                                           const uint32_t *__restrict__ order, uint32_t n_reads, const uint32_t *__restrict__ seg_start, int k,
                                           uint32_t wave, uint32_t n_waves, Op &op) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t total = seg_start[n_reads];
    const u32x4 zero = {0u, 0u, 0u, 0u};
    for (uint32_t sp = wave; sp < total; sp += n_waves) {
        const uint32_t lo_r = span_of(seg_start, n_reads, sp);
        const uint32_t read = order ? order[lo_r] : lo_r;
        const uint32_t len = (uint32_t)lengths[read];  // at least k: the read has a span
        const uint32_t lpad = (len + 15u) & ~15u;
        const uint32_t w0 = (sp - seg_start[lo_r]) * (uint32_t)kScreenSpan;
        const uint32_t w1 = min(len - (uint32_t)k + 1u, w0 + (uint32_t)kScreenSpan);  // this span: window starts [w0, w1)
        const uint8_t *base = plane + offsets[read];

        uint32_t p = w0 + lane * 16u;
        u32x4 a = p < w1 ? *(const u32x4 *)(base + p) : zero;
        u32x4 b = (p < w1 && p + 16u < lpad) ? *(const u32x4 *)(base + p + 16u) : zero;
        u32x4 c = (p < w1 && p + 32u < lpad) ? *(const u32x4 *)(base + p + 32u) : zero;
        uint32_t sum = 0;
        for (uint32_t sb = w0; sb < w1; sb += (uint32_t)kScreenStep, p += (uint32_t)kScreenStep) {
            const uint32_t pn = p + (uint32_t)kScreenStep;  // the next step's bytes, requested before this step's are used
            const bool more = pn < w1;
            const u32x4 na = more ? *(const u32x4 *)(base + pn) : zero;
            const u32x4 nb = (more && pn + 16u < lpad) ? *(const u32x4 *)(base + pn + 16u) : zero;
            const u32x4 nc = (more && pn + 32u < lpad) ? *(const u32x4 *)(base + pn + 32u) : zero;
            if (p < w1) {
                uint64_t hi, lo;
                const uint32_t wv = lane_words(a, b, c, k, w1 - p, &hi, &lo);
                if (wv) sum += op.step(hi, lo, wv);
            }
            a = na;
            b = nb;
            c = nc;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
        if (lane == 0 && sum) op.done(read, sum);
    }
}

__device__ __forceinline__ uint64_t slot_load(const uint64_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the key into the table (never full: the caller grew it); true: it took an empty slot
__device__ __forceinline__ bool table_insert(uint64_t *table, uint64_t mask, uint64_t key) {
    uint64_t s = screenk::mix(key) & mask;
    for (;;) {
        uint64_t v = slot_load(table + s);  // (a stored key never changes: only an empty slot needs the CAS)
        if (v == kEmpty) v = (uint64_t)atomicCAS((unsigned long long *)(table + s), (unsigned long long)kEmpty, (unsigned long long)key);
        if (v == kEmpty) return true;
        if (v == key) return false;
        s = (s + 1ull) & mask;
    }
}

struct InsertOp {
    uint64_t *table;
    uint64_t mask;
    unsigned long long *count;
    int k;
    __device__ __forceinline__ uint32_t step(uint64_t hi, uint64_t lo, uint32_t wv) {
        uint32_t taken = 0;
#pragma unroll
        for (int j = 0; j < 16; ++j)
            if ((wv >> j) & 1u) taken += table_insert(table, mask, window_key(hi, lo, j, k)) ? 1u : 0u;
        return taken;
    }
    __device__ __forceinline__ void done(uint32_t, uint32_t sum) { atomicAdd(count, (unsigned long long)sum); }
};

struct HitsOp {
    const uint64_t *table;
    uint64_t mask;
    uint32_t *hits;
    int k;
    __device__ __forceinline__ uint32_t step(uint64_t hi, uint64_t lo, uint32_t wv) {
        uint32_t count = 0;
#pragma unroll
        for (int g = 0; g < 16; g += kGroup) {
            if (((wv >> g) & ((1u << kGroup) - 1u)) == 0u) continue;
            uint64_t key[kGroup], slot[kGroup], val[kGroup];
#pragma unroll
            for (int j = 0; j < kGroup; ++j) {  // (a window that is not valid issues no request)
                key[j] = window_key(hi, lo, g + j, k);
                slot[j] = screenk::mix(key[j]) & mask;
                val[j] = ((wv >> (g + j)) & 1u) ? table[slot[j]] : kEmpty;
            }
#pragma unroll
            for (int j = 0; j < kGroup; ++j) {
                uint64_t v = val[j], s = slot[j];
                while (v != key[j] && v != kEmpty) {  // (kEmpty is no key: a window that is not valid ends here at once)
                    s = (s + 1ull) & mask;
                    v = table[s];
                }
                count += v == key[j] ? 1u : 0u;
            }
        }
        return count;
    }
    __device__ __forceinline__ void done(uint32_t read, uint32_t sum) { atomicAdd(&hits[read], sum); }
};

__global__ void __launch_bounds__(kHashThreads) k_screenset_insert(const uint8_t *__restrict__ plane, const uint64_t *__restrict__ offsets,
                                                                   const int32_t *__restrict__ lengths, uint32_t n_seqs,
                                                                   const uint32_t *__restrict__ seg_start, int k, uint64_t *table, uint64_t mask,
                                                                   unsigned long long *count) {
    InsertOp op{table, mask, count, k};
    const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * (kHashThreads / 64) + (threadIdx.x >> 6));
    walk_spans(plane, offsets, lengths, nullptr, n_seqs, seg_start, k, wave, gridDim.x * (kHashThreads / 64), op);
}

__global__ void __launch_bounds__(kHashThreads) k_screen_hits_hash(const uint8_t *__restrict__ plane, const uint64_t *__restrict__ offsets,
                                                                   const int32_t *__restrict__ lengths, const uint32_t *__restrict__ order,
                                                                   uint32_t n_reads, const uint32_t *__restrict__ seg_start, int k,
                                                                   const uint64_t *__restrict__ table, uint64_t mask, uint32_t *hits) {
    HitsOp op{table, mask, hits, k};
    const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * (kHashThreads / 64) + (threadIdx.x >> 6));
    walk_spans(plane, offsets, lengths, order, n_reads, seg_start, k, wave, gridDim.x * (kHashThreads / 64), op);
}

__global__ void __launch_bounds__(256) k_screenset_rehash(const uint64_t *__restrict__ from, uint64_t from_capacity, uint64_t *to, uint64_t to_mask) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < from_capacity; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t key = from[i];
        if (key != kEmpty) table_insert(to, to_mask, key);
    }
}

int set_alloc_table(flx_ctx *ctx, uint64_t capacity, uint64_t **out) {
    void *p = nullptr;
    if (capacity > (1ull << 40) || hipMalloc(&p, capacity * 8) != hipSuccess) {
        (void)hipGetLastError();
        return flx_fail(ctx, FLX_ERR_NOMEM, "the screen's table of %llu slots does not fit the device", (unsigned long long)capacity);
    }
    hipError_t e = hipMemsetAsync(p, 0xFF, capacity * 8, ctx->stream);
    if (e != hipSuccess) {
        (void)hipFree(p);
        return flx_fail(ctx, FLX_ERR_HIP, "hipMemsetAsync failed: %s", hipGetErrorString(e));
    }
    *out = (uint64_t *)p;
    return FLX_OK;
}

// the table at `capacity` slots (more than it has), with every stored key; on failure the set is as it was
int set_grow(flx_screenset *set, uint64_t capacity) {
    flx_ctx *ctx = set->ctx;
    uint64_t *to = nullptr;
    FLX_CHECK(set_alloc_table(ctx, capacity, &to));
    if (set->size) {
        const uint64_t blocks = std::min<uint64_t>((set->capacity + 255) / 256, 8ull * (uint64_t)ctx->prop.multiProcessorCount);
        hipLaunchKernelGGL(k_screenset_rehash, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, (const uint64_t *)set->d_table, set->capacity, to,
                           capacity - 1);
    }
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
        (void)hipFree(to);
        return flx_fail(ctx, FLX_ERR_HIP, "rehashing the screen's table failed: %s", hipGetErrorString(e));
    }
    (void)hipFree(set->d_table);
    set->d_table = to;
    set->capacity = capacity;
    return FLX_OK;
}

}  // namespace

bool flx_screenset_is_final(const flx_screenset *set) { return set->final; }

extern "C" int flx_screenset_create(flx_ctx *ctx, int k, int log2_capacity_hint, flx_screenset **out) {
    if (!ctx || !out) return FLX_ERR_INVALID;
    *out = nullptr;
    if (k < screenk::kMinK || k > screenk::kMaxK) return flx_fail(ctx, FLX_ERR_INVALID, "flx_screenset_create: k must be 16..31");
    if (log2_capacity_hint < 1 || log2_capacity_hint > 40) return flx_fail(ctx, FLX_ERR_INVALID, "flx_screenset_create: log2_capacity_hint must be 1..40");
    FLX_HIP(ctx, hipSetDevice(ctx->device));
    flx_screenset *set = new flx_screenset;
    set->ctx = ctx;
    set->k = k;
    set->capacity = 1ull << log2_capacity_hint;
    int rc = set_alloc_table(ctx, set->capacity, &set->d_table);
    if (rc == FLX_OK && hipMalloc((void **)&set->d_count, 8) != hipSuccess) {
        (void)hipGetLastError();
        rc = flx_fail(ctx, FLX_ERR_NOMEM, "flx_screenset_create: no device memory");
    }
    if (rc == FLX_OK && hipMemsetAsync(set->d_count, 0, 8, ctx->stream) != hipSuccess) rc = flx_fail(ctx, FLX_ERR_HIP, "hipMemsetAsync failed");
    int per_cu = 0;
    if (rc == FLX_OK && (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_screen_hits_hash, kHashThreads, 0) != hipSuccess || per_cu < 1))
        per_cu = 1;
    if (rc != FLX_OK) {
        flx_screenset_destroy(set);
        return rc;
    }
    set->blocks = (unsigned)per_cu * (unsigned)ctx->prop.multiProcessorCount;
    *out = set;
    return FLX_OK;
}

extern "C" void flx_screenset_destroy(flx_screenset *set) {
    if (!set) return;
    (void)hipSetDevice(set->ctx->device);
    (void)hipStreamSynchronize(set->ctx->stream);
    if (set->d_table) (void)hipFree(set->d_table);
    if (set->d_count) (void)hipFree(set->d_count);
    delete set;
}

extern "C" int flx_screenset_add(flx_screenset *set, const uint8_t *bases, const uint64_t *offsets, const int64_t *lengths, uint64_t n_seqs) {
    if (!set) return FLX_ERR_INVALID;
    flx_ctx *ctx = set->ctx;
    if (set->final) return flx_fail(ctx, FLX_ERR_STATE, "flx_screenset_add after flx_screenset_finalize");
    if (n_seqs && (!bases || !offsets || !lengths)) return flx_fail(ctx, FLX_ERR_INVALID, "NULL sequence arrays");
    if (n_seqs > 0xfffffffeull) return flx_fail(ctx, FLX_ERR_INVALID, "at most 2^32-2 sequences per call");
    // the sequences that have a window, each at a multiple of 16 of a plane of the batch's own (the caller's offsets may be any):
    // the kernel then loads exactly as the query does.  The padding is zero, which is no base.
    std::vector<uint64_t> at;
    std::vector<int32_t> len;
    std::vector<uint64_t> from;
    uint64_t plane_bytes = 0, windows = 0;
    for (uint64_t i = 0; i < n_seqs; ++i) {
        if (lengths[i] < 0 || lengths[i] > 0x7fffffffll) return flx_fail(ctx, FLX_ERR_INVALID, "sequence %llu: length must be 0 .. 2^31-1", (unsigned long long)i);
        if (lengths[i] < set->k) continue;
        at.push_back(plane_bytes);
        len.push_back((int32_t)lengths[i]);
        from.push_back(offsets[i]);
        plane_bytes += ((uint64_t)lengths[i] + 15) & ~15ull;
        windows += screenk::windows_of(lengths[i], set->k);
    }
    const uint64_t n = at.size();
    if (n == 0) return FLX_OK;
    if (plane_bytes / (uint64_t)kScreenSpan + n > 0xffffffffull) return flx_fail(ctx, FLX_ERR_INVALID, "too many spans in one call");
    FLX_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;

    std::vector<uint8_t> plane(plane_bytes, 0);
    for (uint64_t i = 0; i < n; ++i) memcpy(plane.data() + at[i], bases + from[i], (size_t)len[i]);
    flx_dbuf d_plane, d_off, d_len;
    FLX_CHECK(flx_dalloc(ctx, d_plane, plane_bytes));
    FLX_CHECK(flx_dalloc(ctx, d_off, n * 8));
    FLX_CHECK(flx_dalloc(ctx, d_len, n * 4));
    uint32_t *seg_start = nullptr;
    // every window of the batch may be a new key: the load stays at or below 1/2 whatever it holds
    uint64_t capacity = set->capacity;
    while (capacity < 2 * (set->size + windows)) capacity *= 2;
    if (capacity > set->capacity) FLX_CHECK(set_grow(set, capacity));

    FLX_HIP(ctx, hipMemcpyAsync(d_plane.p, plane.data(), plane_bytes, hipMemcpyHostToDevice, st));
    FLX_HIP(ctx, hipMemcpyAsync(d_off.p, at.data(), n * 8, hipMemcpyHostToDevice, st));
    FLX_HIP(ctx, hipMemcpyAsync(d_len.p, len.data(), n * 4, hipMemcpyHostToDevice, st));
    FLX_CHECK(flx_screen_segment_table(ctx, d_len.as<int32_t>(), nullptr, n, set->k, &seg_start));
    hipLaunchKernelGGL(k_screenset_insert, dim3(set->blocks), dim3(kHashThreads), 0, st, (const uint8_t *)d_plane.p, (const uint64_t *)d_off.p,
                       (const int32_t *)d_len.p, (uint32_t)n, (const uint32_t *)seg_start, set->k, set->d_table, set->capacity - 1,
                       (unsigned long long *)set->d_count);
    FLX_HIP(ctx, hipGetLastError());
    uint64_t size = 0;
    FLX_HIP(ctx, hipMemcpyAsync(&size, set->d_count, 8, hipMemcpyDeviceToHost, st));
    FLX_HIP(ctx, hipStreamSynchronize(st));
    set->size = size;
    return FLX_OK;
}

extern "C" int flx_screenset_finalize(flx_screenset *set) {
    if (!set) return FLX_ERR_INVALID;
    if (set->final) return flx_fail(set->ctx, FLX_ERR_STATE, "flx_screenset_finalize: the set is final already");
    set->final = true;
    return FLX_OK;
}

extern "C" uint64_t flx_screenset_size(const flx_screenset *set) { return set ? set->size : 0; }
extern "C" int flx_screenset_k(const flx_screenset *set) { return set ? set->k : 0; }
extern "C" uint64_t flx_screenset_capacity(const flx_screenset *set) { return set ? set->capacity : 0; }

int flx_screenset_launch_hits(flx_ctx *ctx, const flx_screenset *set, const void *d_plane, const void *d_offsets, const void *d_lengths,
                              const void *d_order, uint64_t n_reads, const uint32_t *seg_start, uint32_t *d_hits) {
    ctx->last_screen_filter = "hash";
    hipLaunchKernelGGL(k_screen_hits_hash, dim3(set->blocks), dim3(kHashThreads), 0, ctx->stream, (const uint8_t *)d_plane, (const uint64_t *)d_offsets,
                       (const int32_t *)d_lengths, (const uint32_t *)d_order, (uint32_t)n_reads, seg_start, set->k, (const uint64_t *)set->d_table,
                       set->capacity - 1, d_hits);
    FLX_HIP(ctx, hipGetLastError());
    return FLX_OK;
}

extern "C" int flx_screenset_hits_dev(flx_ctx *ctx, const flx_screenset *set, const void *d_plane, uint64_t plane_bytes, const void *d_offsets,
                                      const void *d_lengths, const void *d_order, uint64_t n_reads, uint32_t *d_hits) {
    if (!ctx) return FLX_ERR_INVALID;
    if (!set) return flx_fail(ctx, FLX_ERR_INVALID, "flx_screenset_hits: set must not be NULL");
    return screen_hits_dev(ctx, flx_screen_ref{nullptr, set}, d_plane, plane_bytes, d_offsets, d_lengths, d_order, n_reads, d_hits);
}

extern "C" int flx_screenset_hits(flx_ctx *ctx, const flx_screenset *set, const uint8_t *plane, uint64_t plane_bytes, const uint64_t *offsets,
                                  const int32_t *lengths, const uint32_t *order, uint64_t n_reads, uint32_t *hits) {
    if (!ctx) return FLX_ERR_INVALID;
    if (!set) return flx_fail(ctx, FLX_ERR_INVALID, "flx_screenset_hits: set must not be NULL");
    return screen_hits_host(ctx, flx_screen_ref{nullptr, set}, plane, plane_bytes, offsets, lengths, order, n_reads, hits);
}
