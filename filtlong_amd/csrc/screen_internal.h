// screen_internal.h — what screen.hip, screen_hash.hip and pipeline.hip know of each other (host side; the kernels' walk is
// screen_walk.h).
#pragma once

#include "flx_internal.h"
#include "kmerset.h"
#include "screen.h"

bool flx_screenset_is_final(const flx_screenset *set);  // screen_hash.hip

// A set to screen against, not owned: the 16-mer bitmap of flx_screen_set_add or the hashed K-mers of a flx_screenset (one of the two).
struct flx_screen_ref {
    const flx_kmerset *bitmap = nullptr;
    const flx_screenset *hashed = nullptr;
    explicit operator bool() const { return bitmap || hashed; }
    int k() const { return hashed ? flx_screenset_k(hashed) : 16; }
    bool is_final() const { return hashed ? flx_screenset_is_final(hashed) : flx_kmerset_is_final(bitmap); }
    uint64_t size() const { return hashed ? flx_screenset_size(hashed) : flx_kmerset_size(bitmap); }
};

// screen.hip -------------------------------------------------------------------------------------
// The segment table of a walk over windows of k bases: the spans of every read in processing order, scanned.  counts [n + 1] |
// seg_start [n + 1] | the scan's block sums, in the context's scratch; seg_start is filled on the context's stream.  A span is `span`
// window start positions (the screen's kScreenSpan unless the walk has its own: complexity.hip).
int flx_screen_segment_table(flx_ctx *ctx, const int32_t *d_lengths, const uint32_t *d_order, uint64_t n, int k, uint32_t **seg_start,
                             uint32_t span = (uint32_t)screen::kScreenSpan);
// flx_screen_hits_dev / flx_screenset_hits_dev, and their host-array forms, behind the check of their own set's NULL
int screen_hits_dev(flx_ctx *ctx, flx_screen_ref ref, const void *d_plane, uint64_t plane_bytes, const void *d_offsets, const void *d_lengths,
                    const void *d_order, uint64_t n_reads, uint32_t *d_hits);
int screen_hits_host(flx_ctx *ctx, flx_screen_ref ref, const uint8_t *plane, uint64_t plane_bytes, const uint64_t *offsets,
                     const int32_t *lengths, const uint32_t *order, uint64_t n_reads, uint32_t *hits);
// passed[i] = 0 and child_passed = 0 for the children of every read the screen excludes; excluded[i] says which
int flx_screen_apply_dev(flx_ctx *ctx, uint64_t n_reads, const int32_t *d_lengths, const uint32_t *d_hits, uint64_t t, int k,
                         uint8_t *d_passed, const uint64_t *d_child_offsets, uint8_t *d_child_passed, uint8_t *d_excluded);

// screen_hash.hip --------------------------------------------------------------------------------
// k_screen_hits_hash over a finished segment table, on the context's stream
int flx_screenset_launch_hits(flx_ctx *ctx, const flx_screenset *set, const void *d_plane, const void *d_offsets, const void *d_lengths,
                              const void *d_order, uint64_t n_reads, const uint32_t *seg_start, uint32_t *d_hits);
