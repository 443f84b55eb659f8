// adapters.hip — --trim_adapters: where the known adapters end at the two ends of every read (adapters.h has the definition).
//
// Approximate matching of a handful of short patterns against two short texts per read: compute, not bandwidth.
//
//   k_adapter_cuts   the work item is a (read end, pattern) pair, pattern-minor, so the lanes of a wave mostly share one text.  A
//                    workgroup takes `epb` consecutive read ends (end 2 i is the head and end 2 i + 1 the tail of the i-th read in
//                    processing order) and stages their texts once in LDS, one byte a base, already folded to the 2-bit code or
//                    kNoBase; the tail is staged reversed, so both ends run the same loop.  A lane keeps the column of its pattern
//                    in registers (Pv, Mv, the score at row m, dmin, jbest) and its four match masks beside them; the mask of a
//                    text base is chosen by four compare-and-selects, a byte outside ACGTacgt gets the zero mask: no table lookup
//                    per base, no dynamic register indexing, no scratch.  The text comes out of LDS four bases a read (a wave's
//                    lanes on one text read the same dword: a broadcast).  A pattern that hits writes (jbest << 8) | pattern
//                    with one atomicMax into the end's key, zeroed before.
//   --adapter_overhang  an object with O > 0 (flx_adapters_set_overhang) runs the second instantiation, k_adapter_cuts<true>: behind
//                    its free walk a lane whose pattern has O_p > 0 walks the same staged text again from its first base, anchored
//                    (adapters.h), with the same four masks, for min(n, m + k'_p) <= 89 columns, and its one atomicMax takes the
//                    larger of the two candidates.  No LDS and no staging of its own, the same work-item layout.  An object with
//                    O = 0 launches k_adapter_cuts<false>, which has no trace of the second walk.
//   bounds           staging reads the bytes [offset, offset + L) of a read and no other; the keys of read r are 2 r and 2 r + 1.
//   children         k_adapter_children turns the two keys into the child CSR's count, first and last (the rule: adapters.h);
//                    k_adapter_emit writes the one range.  Everything behind that — the child plane, the children's scoring — is
//                    the code --split_window_q runs (qsplit.hip: flx_phred_children).
//   --split_adapters an object with the middle search on (flx_adapters_set_split) takes its children from adapters_split.hip
//                    instead: the keys as before, then the marks over the whole read and the child walk over both.
#include <algorithm>

#include "adapters_internal.h"
#include "rank_internal.h"

using adapters::Pattern;

namespace {

constexpr int kThreads = 256;
constexpr int kLdsTextBytes = 32768;  // of staged texts per workgroup
constexpr int kItemsPerGroup = 1024;  // (read end, pattern) pairs a workgroup aims for: four rounds of its 256 lanes
constexpr int kMaxEnds = 1024;        // read ends per workgroup at most (one pattern)

struct CutArgs {
    const uint8_t *plane;
    const uint64_t *offsets;
    const int32_t *lengths;
    const uint32_t *order;
    uint64_t n_ends;  // 2 * n_reads
    const Pattern *patterns;
    uint32_t n_patterns;
    int32_t w;
    uint32_t stride;  // bytes of LDS per text: round_up(w, 16)
    uint32_t epb;     // read ends per workgroup
    uint32_t *keys;   // [n_ends], zero
};

template <bool kOverhang>
__global__ void __launch_bounds__(kThreads) k_adapter_cuts(const CutArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t s_text[];  // [epb][stride]
    __shared__ int32_t s_n[kMaxEnds];                                  // bases of the text (0: nothing to do)
    __shared__ uint32_t s_read[kMaxEnds];
    const uint64_t e0 = (uint64_t)blockIdx.x * a.epb;

    for (uint32_t le = threadIdx.x; le < a.epb; le += kThreads) {
        const uint64_t ge = e0 + le;
        int32_t n = 0;
        uint32_t read = 0;
        if (ge < a.n_ends) {
            const uint64_t ri = ge >> 1;
            read = a.order ? a.order[ri] : (uint32_t)ri;
            const int32_t l = a.lengths[read];
            n = l < a.w ? l : a.w;
            n = n < 0 ? 0 : n;
        }
        s_n[le] = n;
        s_read[le] = read;
    }
    __syncthreads();

    // the texts: base j of the head is read[j], base j of the tail read[L - 1 - j]; both inside [0, L)
    const uint32_t text_bytes = a.epb * a.stride;
    for (uint32_t idx = threadIdx.x; idx < text_bytes; idx += kThreads) {
        const uint32_t le = idx / a.stride, j = idx - le * a.stride;
        uint32_t code = adapters::kNoBase;
        if ((int32_t)j < s_n[le]) {
            const uint32_t read = s_read[le];
            const int64_t l = a.lengths[read];
            const int64_t pos = ((e0 + le) & 1u) ? l - 1 - (int64_t)j : (int64_t)j;
            code = adapters::code_of(a.plane[a.offsets[read] + (uint64_t)pos]);
        }
        s_text[idx] = (uint8_t)code;
    }
    __syncthreads();

    const uint32_t items = a.epb * a.n_patterns;
    for (uint32_t it = threadIdx.x; it < items; it += kThreads) {
        const uint32_t le = it / a.n_patterns, p = it - le * a.n_patterns;
        const int32_t n = s_n[le];
        if (n == 0) continue;
        const uint32_t side = (uint32_t)((e0 + le) & 1u);
        const Pattern *pat = a.patterns + p;
        const uint64_t *src = side ? pat->peq_tail : pat->peq_head;
        const uint64_t peq0 = src[0], peq1 = src[1], peq2 = src[2], peq3 = src[3];
        const uint32_t m = pat->m, k = pat->k;
        const uint64_t top = 1ull << (m - 1u);
        adapters::Column col;
        adapters::column_start(&col, m);
        const uint32_t *text = (const uint32_t *)(s_text + le * a.stride);
        for (int32_t j0 = 0; j0 < n; j0 += 4) {
            const uint32_t four = text[j0 >> 2];
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                if (j0 + b < n) {
                    const uint32_t code = (four >> (8 * b)) & 0xffu;
                    uint64_t eq = 0;
                    eq = code == 0u ? peq0 : eq;
                    eq = code == 1u ? peq1 : eq;
                    eq = code == 2u ? peq2 : eq;
                    eq = code == 3u ? peq3 : eq;
                    adapters::column_step(&col, eq, top, j0 + b + 1);
                }
            }
        }
        if constexpr (kOverhang) {
            // the anchored walk: the same text from its first base, the first o pattern bases free
            uint32_t cut = col.dmin <= (int32_t)k ? (uint32_t)col.jbest : 0u;  // (a hit has jbest >= 1)
            const uint32_t o = pat->o;
            if (o != 0u) {
                const uint32_t k_o = pat->k_o;
                const int32_t cols = adapters::anchored_columns(n, m, k_o);
                adapters::column_start_anchored(&col, m, o);
                for (int32_t j0 = 0; j0 < cols; j0 += 4) {
                    const uint32_t four = text[j0 >> 2];
#pragma unroll
                    for (int b = 0; b < 4; ++b) {
                        if (j0 + b < cols) {
                            const uint32_t code = (four >> (8 * b)) & 0xffu;
                            uint64_t eq = 0;
                            eq = code == 0u ? peq0 : eq;
                            eq = code == 1u ? peq1 : eq;
                            eq = code == 2u ? peq2 : eq;
                            eq = code == 3u ? peq3 : eq;
                            adapters::column_step_anchored(&col, eq, top, j0 + b + 1);
                        }
                    }
                }
                if (col.dmin <= (int32_t)k_o && (uint32_t)col.jbest > cut) cut = (uint32_t)col.jbest;
            }
            if (cut) atomicMax(&a.keys[2ull * s_read[le] + side], (cut << 8) | p);
        } else {
            if (col.dmin <= (int32_t)k) atomicMax(&a.keys[2ull * s_read[le] + side], ((uint32_t)col.jbest << 8) | p);
        }
    }
}

// per read: children (0 or 1), first and last; n_child[n_reads] = 0 (the scan's last entry is the total)
__global__ void __launch_bounds__(256) k_adapter_children(uint64_t n_reads, const int32_t *lengths, const uint32_t *keys, int64_t *n_child,
                                                          int32_t *first, int32_t *last) {
    const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (r > n_reads) return;
    if (r == n_reads) {
        n_child[r] = 0;
        return;
    }
    const int32_t l = lengths[r];
    int32_t f, e;
    n_child[r] = adapters::child_of(keys[2 * r], keys[2 * r + 1], l < 0 ? 0 : l, &f, &e);
    first[r] = f;
    last[r] = e;
}

__global__ void __launch_bounds__(256) k_adapter_emit(uint64_t n_reads, const uint64_t *child_offsets, const int32_t *first, const int32_t *last,
                                                      uint64_t capacity, int32_t *child_ranges, uint32_t *child_parent) {
    const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n_reads) return;
    const uint64_t at = child_offsets[r];
    if (child_offsets[r + 1] == at || at >= capacity) return;
    child_ranges[2 * at] = first[r];
    child_ranges[2 * at + 1] = last[r];
    child_parent[at] = (uint32_t)r;
}

}  // namespace

// the adapters' pattern table on the context's device
int flx_adapters_table(flx_ctx *ctx, flx_adapters *ad, const Pattern **out) {
    std::lock_guard<std::mutex> lk(ad->mu);
    const size_t bytes = ad->patterns.size() * sizeof(Pattern);
    for (auto &d : ad->on_device)
        if (d.device == ctx->device) {
            if (d.version != ad->version) {
                // flx_adapters_set_overhang since the upload: whatever still reads the old table finishes first
                FLX_HIP(ctx, hipSetDevice(ctx->device));
                FLX_HIP(ctx, hipDeviceSynchronize());
                FLX_HIP(ctx, hipMemcpy(d.table, ad->patterns.data(), bytes, hipMemcpyHostToDevice));
                d.version = ad->version;
            }
            *out = d.table;
            return FLX_OK;
        }
    Pattern *p = nullptr;
    FLX_HIP(ctx, hipMalloc((void **)&p, bytes));
    const hipError_t e = hipMemcpy(p, ad->patterns.data(), bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(p);
        return flx_fail(ctx, FLX_ERR_HIP, "the adapters' pattern table: %s", hipGetErrorString(e));
    }
    ad->on_device.push_back({ctx->device, p, ad->version});
    *out = p;
    return FLX_OK;
}

extern "C" int flx_adapters_create(const uint8_t *bases, const uint64_t *offsets, const int64_t *lengths, uint64_t n_seqs, int errors_percent,
                                   int window, flx_adapters **out) {
    if (!out) return FLX_ERR_INVALID;
    *out = nullptr;
    if (n_seqs == 0 || !bases || !offsets || !lengths) return FLX_ERR_INVALID;
    flx_adapters *ad = new flx_adapters();
    if (adapters::build(bases, offsets, lengths, n_seqs, errors_percent, window, &ad->patterns) != 0) {
        delete ad;
        return FLX_ERR_INVALID;
    }
    ad->errors_percent = errors_percent;
    ad->window = window;
    *out = ad;
    return FLX_OK;
}

extern "C" void flx_adapters_destroy(flx_adapters *ad) {
    if (!ad) return;
    for (auto &d : ad->on_device) (void)hipFree(d.table);
    delete ad;
}

extern "C" int flx_adapters_set_overhang(flx_adapters *ad, int overhang) {
    if (!ad) return FLX_ERR_INVALID;
    std::lock_guard<std::mutex> lk(ad->mu);
    if (overhang == ad->overhang) return FLX_OK;
    if (!adapters::set_overhang(&ad->patterns, ad->errors_percent, overhang)) return FLX_ERR_INVALID;
    ad->overhang = overhang;
    ++ad->version;  // a device that holds the table gets it again with its next call (flx_adapters_table)
    return FLX_OK;
}

extern "C" int flx_adapters_overhang(const flx_adapters *ad) { return ad ? ad->overhang : 0; }

extern "C" uint32_t flx_adapters_patterns(const flx_adapters *ad) { return ad ? (uint32_t)ad->patterns.size() : 0u; }

extern "C" int flx_adapter_cuts_dev(flx_ctx *ctx, flx_adapters *ad, const void *d_plane, uint64_t plane_bytes, const void *d_offsets,
                                    const void *d_lengths, const void *d_order, uint64_t n_reads, uint32_t *d_keys) {
    if (!ctx) return FLX_ERR_INVALID;
    if (!ad) return flx_fail(ctx, FLX_ERR_INVALID, "flx_adapter_cuts: adapters must not be NULL");
    if (n_reads > 0x7fffffffull) return flx_fail(ctx, FLX_ERR_INVALID, "at most 2^31-1 reads per batch");
    if (plane_bytes & 15) return flx_fail(ctx, FLX_ERR_INVALID, "plane_bytes must be a multiple of 16");
    if (n_reads == 0) return FLX_OK;
    if (!d_plane || !d_offsets || !d_lengths || !d_keys) return flx_fail(ctx, FLX_ERR_INVALID, "plane/offsets/lengths/keys must not be NULL");
    FLX_HIP(ctx, hipSetDevice(ctx->device));
    CutArgs a;
    memset(&a, 0, sizeof a);
    FLX_CHECK(flx_adapters_table(ctx, ad, &a.patterns));
    a.plane = (const uint8_t *)d_plane;
    a.offsets = (const uint64_t *)d_offsets;
    a.lengths = (const int32_t *)d_lengths;
    a.order = (const uint32_t *)d_order;
    a.n_ends = 2 * n_reads;
    a.n_patterns = (uint32_t)ad->patterns.size();
    a.w = ad->window;
    a.stride = ((uint32_t)ad->window + 15u) & ~15u;
    a.epb = std::max(1u, std::min({(uint32_t)kItemsPerGroup / a.n_patterns, (uint32_t)kLdsTextBytes / a.stride, (uint32_t)kMaxEnds}));
    a.keys = d_keys;
    const uint64_t groups = (a.n_ends + a.epb - 1) / a.epb;  // below 2^32: n_ends is
    flx_time_scope timed(ctx, "flx_adapters");
    FLX_HIP(ctx, hipMemsetAsync(d_keys, 0, a.n_ends * 4, ctx->stream));
    if (ad->overhang > 0)
        hipLaunchKernelGGL(k_adapter_cuts<true>, dim3((unsigned)groups), dim3(kThreads), (size_t)a.epb * a.stride, ctx->stream, a);
    else
        hipLaunchKernelGGL(k_adapter_cuts<false>, dim3((unsigned)groups), dim3(kThreads), (size_t)a.epb * a.stride, ctx->stream, a);
    FLX_HIP(ctx, hipGetLastError());
    timed.end();
    return FLX_OK;
}

extern "C" int flx_adapter_cuts(flx_ctx *ctx, flx_adapters *ad, const uint8_t *plane, uint64_t plane_bytes, const uint64_t *offsets,
                                const int32_t *lengths, const uint32_t *order, uint64_t n_reads, uint32_t *keys) {
    if (!ctx) return FLX_ERR_INVALID;
    if (!ad) return flx_fail(ctx, FLX_ERR_INVALID, "flx_adapter_cuts: adapters must not be NULL");
    if (n_reads > 0x7fffffffull) return flx_fail(ctx, FLX_ERR_INVALID, "at most 2^31-1 reads per batch");
    if (plane_bytes & 15) return flx_fail(ctx, FLX_ERR_INVALID, "plane_bytes must be a multiple of 16");
    if (n_reads == 0) return FLX_OK;
    if (!plane || !offsets || !lengths || !keys) return flx_fail(ctx, FLX_ERR_INVALID, "plane/offsets/lengths/keys must not be NULL");
    FLX_CHECK(flx_check_reads(ctx, plane_bytes, offsets, lengths, order, n_reads));  // (every key is written by the patterns of its own read end)
    FLX_HIP(ctx, hipSetDevice(ctx->device));
    flx_dbuf d_plane, d_off, d_len, d_ord, d_keys;
    FLX_CHECK(flx_dalloc(ctx, d_plane, plane_bytes ? plane_bytes : 16));
    FLX_CHECK(flx_dalloc(ctx, d_off, n_reads * 8));
    FLX_CHECK(flx_dalloc(ctx, d_len, n_reads * 4));
    FLX_CHECK(flx_dalloc(ctx, d_keys, n_reads * 8));
    if (plane_bytes) FLX_HIP(ctx, hipMemcpyAsync(d_plane.p, plane, plane_bytes, hipMemcpyHostToDevice, ctx->stream));
    FLX_HIP(ctx, hipMemcpyAsync(d_off.p, offsets, n_reads * 8, hipMemcpyHostToDevice, ctx->stream));
    FLX_HIP(ctx, hipMemcpyAsync(d_len.p, lengths, n_reads * 4, hipMemcpyHostToDevice, ctx->stream));
    if (order) {
        FLX_CHECK(flx_dalloc(ctx, d_ord, n_reads * 4));
        FLX_HIP(ctx, hipMemcpyAsync(d_ord.p, order, n_reads * 4, hipMemcpyHostToDevice, ctx->stream));
    }
    // (a pattern no key can be: a kernel that wrote nothing must not hand back an earlier call's answers — score_api.hip)
    FLX_HIP(ctx, hipMemsetAsync(d_keys.p, 0xA5, n_reads * 8, ctx->stream));
    FLX_CHECK(flx_adapter_cuts_dev(ctx, ad, d_plane.p, plane_bytes, d_off.p, d_len.p, order ? d_ord.p : nullptr, n_reads, d_keys.as<uint32_t>()));
    FLX_HIP(ctx, hipMemcpyAsync(keys, d_keys.p, n_reads * 8, hipMemcpyDeviceToHost, ctx->stream));
    FLX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return FLX_OK;
}

// flx_score_batch_adapters_dev; the keys stay in d_keys_out when that is not NULL (pipeline.hip)
int flx_adapters_score_dev(flx_ctx *ctx, flx_adapters *ad, const void *d_plane, const void *d_seq_plane, uint64_t plane_bytes, const void *d_offsets,
                           const void *d_lengths, const void *d_order, uint64_t n_reads, const flx_params *params, flx_scores *out,
                           uint32_t *d_keys_out) {
    if (!ctx) return FLX_ERR_INVALID;
    if (!ad) return flx_fail(ctx, FLX_ERR_INVALID, "flx_score_batch_adapters: adapters must not be NULL");
    if (!params || !out) return flx_fail(ctx, FLX_ERR_INVALID, "params/out must not be NULL");
    if (n_reads > 0x7fffffffull) return flx_fail(ctx, FLX_ERR_INVALID, "at most 2^31-1 reads per batch");
    if (plane_bytes & 15) return flx_fail(ctx, FLX_ERR_INVALID, "plane_bytes must be a multiple of 16");
    if (n_reads && (!out->mean_q || !out->window_q || !out->passed))
        return flx_fail(ctx, FLX_ERR_INVALID, "mean_q/window_q/passed outputs are required");
    if (params->window_size <= 0) return flx_fail(ctx, FLX_ERR_INVALID, "window_size must be positive");
    if (params->trim || params->split_set) return flx_fail(ctx, FLX_ERR_INVALID, "trim/split need a k-mer set: not with adapters");
    if (!out->child_offsets) return flx_fail(ctx, FLX_ERR_INVALID, "adapters requested but child_offsets is NULL");
    out->n_children = 0;
    if (n_reads == 0) return FLX_OK;
    if (!d_plane || !d_seq_plane) return flx_fail(ctx, FLX_ERR_INVALID, "the quality plane and the sequence plane must not be NULL");
    FLX_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
    char *wp = nullptr;
    auto carve = [&](size_t bytes) { void *p = wp; wp += up(bytes); return p; };

    // ---- per-read arrays (workspace 0) ----
    const size_t scan_ws = flx_radix_sort_workspace(n_reads + 1);
    void *small = nullptr;
    // (an object with the middle search on: the mark bitmap and the scratch of its kernels behind the rest)
    const int e2 = ad->split_errors_percent;
    const size_t mark_bytes = e2 >= 0 ? adapters::mark_words(plane_bytes) * 4 : 0;
    const size_t split_room = e2 >= 0 ? up(mark_bytes) + up(flx_adapter_marks_scratch(n_reads)) : 0;
    FLX_CHECK(flx_workspace(ctx, 0, up((n_reads + 1) * 8) + 2 * up(n_reads * 4) + up(n_reads * 8) + up(scan_ws) + split_room, &small));
    wp = (char *)small;
    int64_t *d_nchild = (int64_t *)carve((n_reads + 1) * 8);
    int32_t *d_first_tmp = (int32_t *)carve(n_reads * 4), *d_last_tmp = (int32_t *)carve(n_reads * 4);
    uint32_t *d_keys = (uint32_t *)carve(n_reads * 8);
    if (d_keys_out) d_keys = d_keys_out;
    void *d_scanws = carve(scan_ws);
    uint32_t *d_marks = e2 >= 0 ? (uint32_t *)carve(mark_bytes) : nullptr;
    void *d_mark_scratch = e2 >= 0 ? carve(flx_adapter_marks_scratch(n_reads)) : nullptr;
    int32_t *first = out->first ? out->first : d_first_tmp, *last = out->last ? out->last : d_last_tmp;

    // ---- the cuts (and the marks) -> child_offsets ----
    FLX_CHECK(flx_adapter_cuts_dev(ctx, ad, d_seq_plane, plane_bytes, d_offsets, d_lengths, d_order, n_reads, d_keys));
    const unsigned grid = (unsigned)((n_reads + 1 + 255) / 256);
    if (e2 >= 0) {
        FLX_CHECK(flx_adapter_marks_launch(ctx, ad, e2, d_seq_plane, plane_bytes, d_offsets, d_lengths, d_order, n_reads, d_marks, d_mark_scratch));
        FLX_CHECK(flx_adapter_split_launch(ctx, false, n_reads, d_offsets, d_lengths, d_keys, d_marks, d_nchild, first, last, nullptr, 0, nullptr,
                                           nullptr));
    } else {
        hipLaunchKernelGGL(k_adapter_children, dim3(grid), dim3(256), 0, st, n_reads, (const int32_t *)d_lengths, (const uint32_t *)d_keys, d_nchild,
                           first, last);
        FLX_HIP(ctx, hipGetLastError());
    }
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

    return flx_phred_children(ctx, d_plane, plane_bytes, d_offsets, d_lengths, d_order, n_reads, params, out, first, nc, [&](uint32_t *d_parent) {
        if (e2 >= 0)
            return flx_adapter_split_launch(ctx, true, n_reads, d_offsets, d_lengths, d_keys, d_marks, nullptr, nullptr, nullptr,
                                            (const uint64_t *)out->child_offsets, nc, out->child_ranges, d_parent);
        hipLaunchKernelGGL(k_adapter_emit, dim3(grid), dim3(256), 0, st, n_reads, (const uint64_t *)out->child_offsets, (const int32_t *)first,
                           (const int32_t *)last, nc, out->child_ranges, d_parent);
        FLX_HIP(ctx, hipGetLastError());
        return (int)FLX_OK;
    });
}

extern "C" int flx_score_batch_adapters_dev(flx_ctx *ctx, flx_adapters *ad, const void *d_plane, const void *d_seq_plane, uint64_t plane_bytes,
                                            const void *d_offsets, const void *d_lengths, const void *d_order, uint64_t n_reads,
                                            const flx_params *params, flx_scores *out) {
    return flx_adapters_score_dev(ctx, ad, d_plane, d_seq_plane, plane_bytes, d_offsets, d_lengths, d_order, n_reads, params, out, nullptr);
}
