// complexity_internal.h — what complexity.hip and pipeline.hip know of each other (host side; complexity.h has the definition).
#pragma once

#include "flx_internal.h"

#include "complexity.h"

// passed[i] = 0 and child_passed = 0 for the children of every read with (bad << 32) >= t * windows; flagged[i] says which
int flx_complexity_apply_dev(flx_ctx *ctx, uint64_t n_reads, const int32_t *d_lengths, const uint32_t *d_bad, uint64_t t, uint8_t *d_passed,
                             const uint64_t *d_child_offsets, uint8_t *d_child_passed, uint8_t *d_flagged);
