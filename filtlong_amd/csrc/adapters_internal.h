// adapters_internal.h — what adapters.hip (the read ends) and adapters_split.hip (the middle of the reads) share.
#pragma once
#include <mutex>
#include <utility>
#include <vector>

#include "flx_internal.h"
#include "adapters.h"

struct flx_adapters {
    std::vector<adapters::Pattern> patterns;
    int errors_percent = 0, window = 0;
    int split_errors_percent = -1;  // flx_adapters_set_split: 0..40 the middle search is on, -1 off
    int overhang = 0;               // flx_adapters_set_overhang: O, 0 off; o and k_o of every pattern follow it
    uint64_t version = 0;           // of the patterns: counts the changes of `overhang`
    std::mutex mu;
    struct OnDevice {
        int device;
        adapters::Pattern *table;
        uint64_t version;  // of the patterns it holds
    };
    std::vector<OnDevice> on_device;  // the pattern table, uploaded once per device that asks for it and again after a change
};

// the adapters' pattern table on the context's device
int flx_adapters_table(flx_ctx *ctx, flx_adapters *ad, const adapters::Pattern **out);

// adapters_split.hip.  The device scratch of one marks call: flx_adapter_marks_scratch(n_reads) bytes.
size_t flx_adapter_marks_scratch(uint64_t n_reads);
// the marks of a batch into d_marks (adapters::mark_words(plane_bytes) words, zeroed here), queued on the context's stream
int flx_adapter_marks_launch(flx_ctx *ctx, flx_adapters *ad, int split_errors_percent, const void *d_plane, uint64_t plane_bytes,
                             const void *d_offsets, const void *d_lengths, const void *d_order, uint64_t n_reads, uint32_t *d_marks, void *d_scratch);
// The child walk over keys and marks.  emit false: n_child [n_reads + 1, the last one 0], first, last.  emit true: child_ranges and
// child_parent of the reads that have children, from child_offsets.
int flx_adapter_split_launch(flx_ctx *ctx, bool emit, uint64_t n_reads, const void *d_offsets, const void *d_lengths, const uint32_t *d_keys,
                             const uint32_t *d_marks, int64_t *d_nchild, int32_t *d_first, int32_t *d_last, const uint64_t *d_child_offsets,
                             uint64_t capacity, int32_t *d_child_ranges, uint32_t *d_child_parent);
