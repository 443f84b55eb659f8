// fold_grid_tab.h — the grid table of a window size and the start of a regime on it, once for host and device: the fold kernels
// (fold_common.h, score_kmer.hip, score_kmer_long.hip) take the table as an argument and begin their regimes with grid_regime_begin;
// tools/sim_fold_grid.cpp and tools/sim_fold_long.cpp compile the same two functions with g++ and hold them against the plain recurrence.
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
// window fills up).  tools/sim_fold_grid.cpp: this file's table and regime on the host against the plain recurrence, 180 000 bit streams x
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

#if defined(__HIPCC__)
#define FLX_GRID_FN __host__ __device__ __forceinline__
#else
#define FLX_GRID_FN static inline
#endif

// One regime: w = wb + c * ds, exactly, while lo <= c <= hi.  ds == 0 (lo > hi): no regime — every word that moves anything is replayed.
struct GridRegime {
    double wb, ds;
    int lo, hi;
};
FLX_GRID_FN double grid_value(const GridRegime &r, int c) { return fma((double)c, r.ds, r.wb); }  // exact: every operand is a multiple of the regime's grid
FLX_GRID_FN int grid_binade(double w) {  // biased exponent of w: its entry of the table is grid_binade(w) - GridTab::e0
    uint64_t bits;
    memcpy(&bits, &w, 8);
    return (int)((bits >> 52) & 0x7ff);
}

// A regime from w on.  (dstar, lv, top) is the table's entry of w's binade, fetched by the caller from wherever it holds the table
// (dstar = 0 where there is none: a tie, or a binade outside the table).
FLX_GRID_FN GridRegime grid_regime_begin(double w, double dstar, double lv, int top, double ws_d) {
    GridRegime r = {w, 0.0, 0x7fffffff, (int)0x80000000};
    if (!(w > 0.0 && dstar > 0.0)) return r;
    // The top: w must not reach a binade on whose grid w_b does NOT lie (its low bits would be rounded away there).  w_b
    // lies on the grid of binade eb + z, z = the trailing zero bits of its mantissa — a window that has once been full
    // (w = 1.0) stays on the grid of [1, 2) whatever is subtracted, d* is a multiple of it — up to the top of the group.
    uint64_t bits;
    memcpy(&bits, &w, 8);
    const int z = __builtin_ctzll((bits & ((1ull << 52) - 1)) | (1ull << 52));
    const int gb = grid_binade(w) + z < top ? grid_binade(w) + z : top;
    const uint64_t ubits = (uint64_t)(gb + 1) << 52;  // uv = 2^(gb + 1): the first value of the binade above the top
    double uv;
    memcpy(&uv, &ubits, 8);
    // smallest c with w + c d* > lv: the estimate (lv - w) * ws is within 1e-9 of (lv - w) / d*, so its floor is the answer or up to
    // two below it; the values themselves decide (w + c d* is exact: a multiple of w's grid).  Strictly above lv: a step that lands
    // exactly ON the bottom of the group's lowest binade has its true value, w - d, a hair below it when d > d* — in the binade
    // underneath, which rounds on its own, finer grid.
    int k0 = (int)floor((lv - w) * ws_d);
    if (fma((double)k0, dstar, w) <= lv) ++k0;
    if (fma((double)k0, dstar, w) <= lv) ++k0;
    // largest c with w + c d* < uv: the ceiling of the estimate is the answer or up to two above it
    int k1 = (int)ceil((uv - w) * ws_d);
    if (fma((double)k1, dstar, w) >= uv) --k1;
    if (fma((double)k1, dstar, w) >= uv) --k1;
    r.ds = dstar;
    r.lo = k0;
    r.hi = k1;
    return r;
}
// ... with the table held as GridTab (the host simulations); `binade_top`: the regime's top is the binade w is in, not the grid it
// lies on — the rule that lost (tools/sim_fold_grid.cpp counts what it costs)
static inline GridRegime grid_regime_begin(const GridTab &t, double w, double ws_d, bool binade_top = false) {
    const int idx = grid_binade(w) - t.e0;
    if (idx < 0 || idx >= t.n) return grid_regime_begin(w, 0.0, 0.0, 0, ws_d);
    return grid_regime_begin(w, t.dstar[idx], t.lv[idx], binade_top ? grid_binade(w) : t.top[idx], ws_d);
}
