// screen.h — --exclude: reads that match a contaminant reference are dropped.  The host core of screen.hip, and like qsplit.h plain
// C++ that a HIP kernel and a host program both include.  The reference has no counterpart: its users run a second tool (NanoLyse for
// the lambda control strand, chopper --contam) over the whole file in front of it.
//
// Everything is defined on integers, so any decomposition (spans, waves, lanes, chunks, ranks) gives the same answer.
//   the set X     every 16-mer of both strands of the contaminant that consists of ACGTacgt only.  The reference's encoder turns any
//                 other byte into A (src/kmers.cpp:176-219), so an N run handed to flx_kmerset_add_assembly as it is would put poly-A
//                 into X and every poly-A tail would count as a hit: split_acgt below cuts every sequence at the bytes outside
//                 ACGTacgt, and only the pieces of at least 16 bases go into the set, as sequences of their own.
//   hits          for a read of L bases, windows = max(0, L - 15); hits counts the i in [0, windows) for which all 16 bytes
//                 s[i..i+15] are in ACGTacgt and the forward 2-bit code of the window (A 0, C 1, G 2, T 3, first base on top, as
//                 flx_kmerset_contains takes it) is a member of X.
//   threshold     t = (uint64_t)ceil(P / 100 * 2^32) in IEEE double, 0 < P <= 100 (--exclude_percent)
//   decision      a read is excluded iff windows > 0 and (hits << 32) >= t * windows, both in uint64 (both stay below 2^63).
#pragma once

#include <math.h>
#include <stdint.h>

#include <vector>

#if defined(__HIPCC__)
#define SCREEN_FN __host__ __device__ __forceinline__
#else
#define SCREEN_FN inline
#endif

namespace screen {

// The work item of k_screen_hits: this many window start positions of one read (a multiple of kScreenStep).  A 4 Mbp read is
// a thousand items, a 10 kbp read three.
constexpr int kScreenSpan = 4096;
// positions a wave takes per step: 64 lanes with 16 consecutive window starts each
constexpr int kScreenStep = 1024;
static_assert(kScreenSpan % kScreenStep == 0, "a span is whole steps");

SCREEN_FN bool is_acgt(uint8_t c) {
    const uint32_t d = (uint32_t)(c | 0x20u) - 0x61u;  // a 0, c 2, g 6, t 19
    return d < 32u && ((0x80045u >> d) & 1u);
}
// A 0, C 1, G 2, T 3 for a byte of ACGTacgt (any value for another byte: the caller masks those windows)
SCREEN_FN uint32_t code_of(uint8_t c) { return ((c >> 1) ^ (c >> 2)) & 3u; }

SCREEN_FN uint32_t windows_of(int64_t length) { return length > 15 ? (uint32_t)(length - 15) : 0u; }

SCREEN_FN bool excluded(uint32_t hits, uint32_t windows, uint64_t t) {
    return windows > 0 && ((uint64_t)hits << 32) >= t * (uint64_t)windows;
}

// t of --exclude_percent P; false unless 0 < P <= 100
inline bool threshold(double percent, uint64_t *t) {
    if (!(percent > 0.0 && percent <= 100.0)) return false;
    volatile double frac = percent / 100.0;  // (rounded to double before the product, whatever the host's evaluation mode)
    volatile double scaled = frac * 4294967296.0;
    *t = (uint64_t)ceil(scaled);  // positive and at most 2^32
    return true;
}

// The ACGT-only pieces of at least 16 bases of the sequences bases[offsets[i] .. offsets[i] + lengths[i]), in order, as offsets into
// `bases` and lengths: what goes into the set.  Reads the sequences' bytes and nothing else.
inline void split_acgt(const uint8_t *bases, const uint64_t *offsets, const int64_t *lengths, uint64_t n_seqs,
                       std::vector<uint64_t> *piece_offsets, std::vector<int64_t> *piece_lengths) {
    piece_offsets->clear();
    piece_lengths->clear();
    for (uint64_t s = 0; s < n_seqs; ++s) {
        const uint64_t begin = offsets[s], end = begin + (uint64_t)(lengths[s] > 0 ? lengths[s] : 0);
        uint64_t run = begin;  // start of the current run of ACGT bytes
        for (uint64_t i = begin; i <= end; ++i) {
            if (i < end && is_acgt(bases[i])) continue;
            if (i - run >= 16) {
                piece_offsets->push_back(run);
                piece_lengths->push_back((int64_t)(i - run));
            }
            run = i + 1;
        }
    }
}

}  // namespace screen
