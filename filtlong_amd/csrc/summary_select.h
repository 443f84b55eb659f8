// summary_select.h — the host side of flx_summary's order statistics (summary.hip): which digit each of the ten targets
// takes after a radix pass, and what it carries into the next one.  Plain C++, no HIP: tests/summary_select_host.cpp drives it
// with histograms computed on the host.
//
// The counted entries are thought of in DESCENDING order of length.  The ten targets are
//     t = 0..8   N10, N20, ... N90: the length of the first entry at which 100 * cum >= x * bases, x = 10 (t + 1), where cum is
//                the sum of the lengths up to and including that entry (0 when bases == 0);
//     t = 9      the median: entry (n - 1) / 2 of the ASCENDING order = entry n / 2 of the descending one, i.e. the first
//                entry at which the number of entries up to and including it reaches n / 2 + 1 (0 when n == 0).
// The 32-bit length is resolved 8 bits per pass from the top, in four passes.  Before a pass every target knows the bits it
// has fixed so far (its prefix) and what lies strictly above that prefix (entries and bases).  The pass needs, for every
// DISTINCT prefix still alive, the 256-bin histogram (entries, bases) of the next digit over the entries below that prefix: at
// most ten rows, and targets with the same prefix share a row (targets are not distinct: all-equal lengths keep all ten in one
// row through all four passes).  Histograms of several ranks are summed bin by bin before the step; nothing else is exchanged.
// 100 * cum and x * bases are carried in 128 bits: bases is any 64-bit sum.
#pragma once
#include <cstdint>

namespace flx_summary_select {

constexpr int kTargets = 10;        // N10 .. N90, median
constexpr int kMedian = 9;
constexpr int kPasses = 4;          // 8 bits each, from the top
constexpr int kDigits = 256;
// the launch shape of both kernels of summary.hip: at most kMaxBlocks workgroups of kThreads threads walk the entries in a
// grid-stride loop (one sweep of the full grid = kMaxBlocks * kThreads entries)
constexpr int kThreads = 256;
constexpr int kMaxBlocks = 512;

struct Bin {
    uint64_t count, bases;
};

struct State {
    uint64_t n = 0, bases = 0;
    int pass = 0;                        // passes done
    uint32_t prefix[kTargets];           // the top 8 * pass bits of the target's length
    uint64_t above_count[kTargets];      // entries whose top bits are strictly greater than the prefix
    uint64_t above_bases[kTargets];      // ... and the sum of their lengths
    int row[kTargets];                   // the histogram row of the target in the coming pass
    int n_rows = 0;
    uint32_t row_prefix[kTargets];       // the prefix every row stands for
    bool consistent = true;              // false once a histogram did not hold the entry a target was looking for
};

inline void assign_rows(State &s) {
    s.n_rows = 0;
    for (int t = 0; t < kTargets; ++t) {
        int r = 0;
        while (r < s.n_rows && s.row_prefix[r] != s.prefix[t]) ++r;
        if (r == s.n_rows) s.row_prefix[s.n_rows++] = s.prefix[t];
        s.row[t] = r;
    }
}

inline void init(State &s, uint64_t n, uint64_t bases) {
    s = State();
    s.n = n;
    s.bases = bases;
    for (int t = 0; t < kTargets; ++t) s.prefix[t] = 0, s.above_count[t] = 0, s.above_bases[t] = 0;
    assign_rows(s);
}

// the shift that brings the digit of the coming pass to the low byte; the prefix of an entry is (uint64_t)length >> (shift + 8)
inline int shift_of(const State &s) { return 8 * (kPasses - 1 - s.pass); }

// has the target been reached once `count` entries and `bases` bases are behind us?
inline bool reached(const State &s, int t, uint64_t count, uint64_t bases) {
    if (t == kMedian) return count >= s.n / 2 + 1;
    return (unsigned __int128)100 * bases >= (unsigned __int128)(10 * (t + 1)) * s.bases;
}

// hist: n_rows rows of 256 bins, row r = the entries whose prefix is row_prefix[r], binned by the digit of this pass
inline void step(State &s, const Bin *hist) {
    for (int t = 0; t < kTargets; ++t) {
        const Bin *h = hist + (uint64_t)s.row[t] * kDigits;
        uint64_t c = s.above_count[t], b = s.above_bases[t];
        int d = kDigits - 1;
        for (;; --d) {
            // (an empty bin cannot be where a target is reached: with bases == 0 every Nx would otherwise stop at digit 255)
            if (h[d].count && reached(s, t, c + h[d].count, b + h[d].bases)) break;
            c += h[d].count;
            b += h[d].bases;
            if (d == 0) {  // not in this row: n == 0, or histograms that do not belong to (n, bases)
                if (s.n) s.consistent = false;
                c = s.above_count[t], b = s.above_bases[t];
                d = 0;
                break;
            }
        }
        s.above_count[t] = c;
        s.above_bases[t] = b;
        s.prefix[t] = (s.prefix[t] << 8) | (uint32_t)d;
    }
    ++s.pass;
    if (s.pass < kPasses) assign_rows(s);
}

// after the four passes
inline int32_t value(const State &s, int t) {
    if (s.n == 0 || (t != kMedian && s.bases == 0)) return 0;
    return (int32_t)s.prefix[t];
}

}  // namespace flx_summary_select
