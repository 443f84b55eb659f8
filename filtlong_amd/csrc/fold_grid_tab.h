// fold_grid_tab.h — the grid table of a window size (plain C++: the fold kernels of score_kmer.hip and score_kmer_long.hip take it as
// an argument, tools/sim_fold_long.cpp builds the same one on the host).
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>

// ---- the window recurrence on the integer grid (round 5) ------------------------------------------------------------------------
// src/read.cpp:228-231 with qualities 0.0 / 1.0 is  w = fl(fl(w - tb * d) + lb * d),  d = fl(1 / ws), and the drift of those
// roundings is part of the result.  But WHERE w rounds is known: on the grid of its binade.  Let d_E be d rounded to the grid of
// binade E (2^(E-52)); a GROUP is a run of binades on which d_E is the same real number d* (and no binade rounds d on a tie).  While
//   * w stays strictly above the bottom of its group (and above 4 d: a step that takes a base out and puts one in dips by d, and the
//     way back is only exact from at most one binade down), and
//   * w does not reach a binade above the one it was in when the regime began (there w's own low bits would be rounded away),
// every step is EXACT:  w = w_b + c * d*  with c the number of covered bases that entered the window minus those that left — all
// operands are multiples of the regime's grid, nothing rounds.  A word of 32 positions then is three small integers — the total,
// the lowest and the highest prefix of its +-1 walk (a table over the (new, old) nibble pairs in LDS) — two compares and two adds;
// the minimum of w over the word is w_b + (lowest prefix) * d*.  A word that leaves the regime is replayed in floating point, FOR
// THAT LANE (the others keep their integer step), and the regime begins again from the value it ends on.  ws = 250 (the default):
// d* = d + 4 ulp on every binade from 2^-4 up, so one regime holds while 16 of the 250 bases are covered and w has been as high
// before; on the synthetic reads 0.7 % of a lane's words are replayed (the way into and out of a junk block, the first time a read's
// window fills up).  tools/sim_fold_grid.cpp: the same regime logic on the host against the plain recurrence, 180 000 bit streams x
// 6000 window sizes, bit for bit — and the tests hold this kernel against the FP kernel (FLX_KMER_FOLD_GRID=0) on every read and child.
struct GridTab {
    enum { kMax = 26 };
    double dstar[kMax];  // per binade of w (biased exponent e0 + i): d on that binade's grid; 0 = no regime there (a tie, or outside)
    double lv[kMax];     // the value w must stay strictly above: max(bottom of the binade's group, 4 d)
    int top[kMax];       // biased exponent of the highest binade of the binade's group
    int e0, n;
};

// The grid table of a window size: per binade of w the step d rounded to that binade's grid, the groups of binades
// that share it, and whether the integer-grid steady state pays — the group that holds [1, 2) must reach down to 2^-3 at least (ws =
// 250: 2^-4; ws = 1000: d rounds differently on either side of 1.0, where the window of a clean read sits — the FP kernel then).
static inline bool build_grid_table(int ws, GridTab &g) {
    memset(&g, 0, sizeof g);
    if (ws < 8 || ws > (1 << 20)) return false;
    volatile double one = 1.0, wsd = (double)ws;
    const double delta = one / wsd;
    uint64_t bits;
    memcpy(&bits, &delta, 8);
    const int e_d = (int)((bits >> 52) & 0x7ff) - 1023;
    const uint64_t M = (bits & ((1ull << 52) - 1)) | (1ull << 52);  // delta = M * 2^(e_d - 52)
    const int e_min = e_d - 2, e_max = 1;
    const int n = e_max - e_min + 1;
    if (n > GridTab::kMax) return false;
    bool tie[GridTab::kMax];
    for (int i = 0; i < n; ++i) {
        const int shift = (e_min + i) - e_d;  // the grid of binade E is 2^shift ulps of delta
        tie[i] = false;
        if (shift <= 0) {
            g.dstar[i] = delta;
        } else {
            const uint64_t rem = M & ((1ull << shift) - 1), half = 1ull << (shift - 1);
            tie[i] = rem == half;
            g.dstar[i] = ldexp((double)((M >> shift) + (rem > half ? 1 : 0)), shift + e_d - 52);
        }
    }
    bool pays = false;
    for (int i = 0; i < n;) {  // groups: maximal runs of binades without a tie that share d*
        if (tie[i]) { g.dstar[i] = 0.0; g.lv[i] = 0.0; ++i; continue; }
        int j = i;
        while (j + 1 < n && !tie[j + 1] && g.dstar[j + 1] == g.dstar[i]) ++j;
        const double bottom = std::max(ldexp(1.0, e_min + i), 4.0 * delta);
        for (int k = i; k <= j; ++k) {
            g.lv[k] = bottom;
            g.top[k] = 1023 + e_min + j;
        }
        if (e_min + i <= -3 && e_min + j >= 0) pays = true;
        i = j + 1;
    }
    g.e0 = 1023 + e_min;
    g.n = n;
    return pays;
}
