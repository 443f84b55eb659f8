// sim_fold_long.cpp — the cooperative window fold of ultra-long reads in k-mer mode (filtlong_amd/csrc/score_kmer_long.hip),
// on the host: the chunked walk against the plain recurrence, bit for bit in w and mn.
//
// The kernel's steps, with a wave's 64 lanes as a loop:
//   * a segment is bits [start, start + len) of a row of 32-bit words; its steps of 32 positions are the leading word (positions
//     ws + 32 k ..) and the trailing word (positions 32 k ..), funnel-shifted out of the row, and their summary (total, lowest and
//     highest prefix of the +-1 walk, a flag for "not all zero", a flag for the partial last word);
//   * the head is (double)popcount(first ws bits) / ws;
//   * 64 summaries at a time: prefix of the totals, every word tested against the regime's bounds (same grid table and the same
//     begin of a regime as both kernels — their own code: filtlong_amd/csrc/fold_grid_tab.h), the first failing word replayed in
//     floating point (the 32 fma pairs), a new regime, the rest of the 64 tested again without recomputing them.
// Reference semantics: src/read.cpp:216-236 with qualities 0.0 / 1.0.
//
// usage: sim_fold_long [random streams per window size]     (exit status 1 on a mismatch)
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../filtlong_amd/csrc/fold_grid_tab.h"

struct Fold { double w, mn; };

// plain recurrence over the bits of the segment
static Fold fold_plain(const std::vector<uint8_t> &q, int ws) {
    const int L = (int)q.size();
    volatile double one = 1.0, wsd = (double)ws;
    const double d = one / wsd;
    if (L < ws) return {0.0, 0.0};
    long cnt = 0;
    for (int i = 0; i < ws; ++i) cnt += q[i];
    double w = (double)cnt / wsd, mn = w;
    for (int j = ws; j < L; ++j) {
        w -= q[j - ws] ? d : 0.0;
        w += q[j] ? d : 0.0;
        if (w < mn) mn = w;
    }
    return {w, mn};
}

struct Seg { const uint32_t *row; int row_words, start, len; };

static uint32_t alignbit(uint32_t hi, uint32_t lo, unsigned s) { return (uint32_t)((((uint64_t)hi << 32) | lo) >> (s & 31u)); }

static uint32_t seg_bits32(const Seg &s, int p) {  // score_kmer_long.hip: seg_bits32
    if (p >= s.len) return 0u;
    const int b = s.start + p, w = b >> 5;
    const uint32_t lo = w < s.row_words ? s.row[w] : 0u, hi = w + 1 < s.row_words ? s.row[w + 1] : 0u;
    uint32_t v = alignbit(hi, lo, (unsigned)(b & 31));
    const int valid = s.len - p;
    if (valid < 32) v &= (1u << valid) - 1u;
    return v;
}

constexpr uint32_t kNonZero = 1u << 24, kPartial = 2u << 24;
static uint32_t g_walk[256];
static void make_walk() {
    for (int idx = 0; idx < 256; ++idx) {
        int t = 0, mp = 0, xp = 0;
        for (int i = 0; i < 4; ++i) {
            t += ((idx >> (4 + i)) & 1) - ((idx >> i) & 1);
            mp = std::min(mp, t);
            xp = std::max(xp, t);
        }
        g_walk[idx] = ((uint32_t)t & 0xffu) | (((uint32_t)mp & 0xffu) << 8) | ((uint32_t)xp << 16);
    }
}

static long g_words = 0, g_replayed = 0;

// the chunked walk (k_kmer_long_words + k_kmer_long_walk)
static Fold fold_long(const Seg &s, int ws, const GridTab &gt) {
    volatile double one = 1.0, wsd_v = (double)ws;
    const double delta = one / wsd_v, ws_d = (double)ws;
    const int len = s.len;
    if (len < ws) return {0.0, 0.0};
    // 1. summaries
    const int nw = len > ws ? (len - ws + 31) >> 5 : 0;
    std::vector<uint32_t> sum((size_t)nw), lw((size_t)nw), tw((size_t)nw);
    for (int k = 0; k < nw; ++k) {
        const int valid = len - ws - 32 * k;
        const uint32_t lead = seg_bits32(s, ws + 32 * k);
        uint32_t trail = seg_bits32(s, 32 * k);
        if (valid < 32) trail &= (1u << valid) - 1u;
        int run = 0, lo = 0, hi = 0;
        for (int q = 0; q < 8; ++q) {
            const uint32_t e = g_walk[(((lead >> (4 * q)) & 15u) << 4) | ((trail >> (4 * q)) & 15u)];
            lo = std::min(lo, run + (int)(int8_t)(e >> 8));
            hi = std::max(hi, run + (int)(e >> 16));
            run += (int)(int8_t)e;
        }
        uint32_t v = ((uint32_t)run & 0xffu) | (((uint32_t)lo & 0xffu) << 8) | ((uint32_t)hi << 16);
        if (lead | trail) v |= kNonZero;
        if (valid < 32) v |= kPartial;
        sum[(size_t)k] = v; lw[(size_t)k] = lead; tw[(size_t)k] = trail;
    }
    // 2. head
    int c0 = 0;
    for (int p = 0; p < ws; p += 32) {
        uint32_t v = seg_bits32(s, p);
        if (ws - p < 32) v &= (1u << (ws - p)) - 1u;
        c0 += __builtin_popcount(v);
    }
    double w = (double)c0 / ws_d, mn = w;
    // the regime (fold_grid_tab.h: the kernel's own start of a regime, the table held as GridTab)
    GridRegime r;
    int c = 0, cmin = 0x7fffffff;
    auto begin = [&]() {
        r = grid_regime_begin(gt, w, ws_d);
        c = 0;
        cmin = 0x7fffffff;
    };
    auto flush = [&]() {
        if (cmin != 0x7fffffff) mn = fmin(mn, grid_value(r, cmin));
        w = grid_value(r, c);
    };
    begin();
    g_words += nw;
    for (int k0 = 0; k0 < nw; k0 += 64) {
        uint32_t sv[64];
        int t[64], mp[64], xp[64], pre[64], incl[64];
        bool any = false;
        for (int l = 0; l < 64; ++l) {
            sv[l] = k0 + l < nw ? sum[(size_t)(k0 + l)] : 0u;
            any = any || (sv[l] & kNonZero);
        }
        if (!any) continue;
        int run = 0;
        for (int l = 0; l < 64; ++l) {
            t[l] = (int)(int8_t)sv[l]; mp[l] = (int)(int8_t)(sv[l] >> 8); xp[l] = (int)((sv[l] >> 16) & 0xffu);
            pre[l] = run; run += t[l]; incl[l] = run;
        }
        int from = 0, pre_from = 0;
        for (;;) {
            int fail = 64;
            for (int l = from; l < 64; ++l) {
                const int ci = c + (pre[l] - pre_from);
                const bool ok = !(sv[l] & kNonZero) || (!(sv[l] & kPartial) && ci + mp[l] >= r.lo && ci + xp[l] <= r.hi);
                if (!ok) { fail = l; break; }
            }
            for (int l = from; l < fail; ++l) cmin = std::min(cmin, c + (pre[l] - pre_from) + mp[l]);
            if (fail == 64) { c += incl[63] - pre_from; break; }
            c += pre[fail] - pre_from;
            flush();
            const uint32_t rl = lw[(size_t)(k0 + fail)], rt = tw[(size_t)(k0 + fail)];
            for (int i = 0; i < 32; ++i) {  // (fold_common.h: fold_word_fp — a device function, so its fma pairs are restated here)
                const double lb = (double)((rl >> i) & 1u), tb = (double)((rt >> i) & 1u);
                w = fma(tb, -delta, w);
                w = fma(lb, delta, w);
                mn = fmin(mn, w);
            }
            ++g_replayed;
            begin();
            pre_from = incl[fail];
            from = fail + 1;
            if (from == 64) break;
        }
    }
    flush();
    return {w, mn};
}

static long g_cases = 0, g_bad = 0;
static std::mt19937_64 g_rng(20240607);

// the stream as a segment at a random bit offset inside a row with other bits around it, and as a read of its own (offset 0)
static void check(const std::vector<uint8_t> &q, int ws, const GridTab &gt, const char *what) {
    const int L = (int)q.size();
    if (L < ws) return;
    const Fold a = fold_plain(q, ws);
    for (int variant = 0; variant < 2; ++variant) {
        const int start = variant ? (int)(g_rng() % 200) : 0, after = variant ? (int)(g_rng() % 100) : 0;
        const int row_len = start + L + after;
        std::vector<uint32_t> row((size_t)((row_len + 31) >> 5) + 1, 0u);
        for (int i = 0; i < row_len; ++i) {
            const bool bit = (i >= start && i < start + L) ? q[(size_t)(i - start)] != 0 : (g_rng() & 1);
            if (bit) row[(size_t)(i >> 5)] |= 1u << (i & 31);
        }
        const Seg s = {row.data(), (row_len + 31) >> 5, start, L};
        const Fold b = fold_long(s, ws, gt);
        ++g_cases;
        if (memcmp(&a.w, &b.w, 8) || memcmp(&a.mn, &b.mn, 8)) {
            if (++g_bad < 10) printf("MISMATCH %s ws %d L %d start %d: w %a vs %a  mn %a vs %a\n", what, ws, L, start, a.w, b.w, a.mn, b.mn);
        }
    }
}

int main(int argc, char **argv) {
    const int n_random = argc > 1 ? atoi(argv[1]) : 60;
    make_walk();
    static const int periods[20][2] = {{16, 16}, {17, 15}, {40, 40}, {100, 20}, {20, 100}, {125, 125}, {126, 124}, {250, 250}, {500, 300}, {62, 190},
                                       {31, 219}, {15, 235}, {8, 242}, {3000, 900}, {1000, 16}, {249, 1}, {1, 16}, {64, 64}, {33, 31}, {700, 700}};
    for (int ws : {8, 64, 128, 250, 500, 333, 2047}) {
        GridTab gt;
        const bool pays = build_grid_table(ws, gt);
        const long words0 = g_words, rep0 = g_replayed;
        // engineered: clean / junk periods (the window count hovers on the regime's edges), with a random phase
        for (int k = 0; k < 20; ++k)
            for (int rep = 0; rep < 3; ++rep) {
                const int L = ws + 2000 + (int)(g_rng() % 20000);
                std::vector<uint8_t> q((size_t)L, 1);
                int pos = (int)(g_rng() % (uint64_t)(periods[k][0] + periods[k][1]));
                while (pos < L) {
                    pos += periods[k][0];
                    for (int i = pos; i < std::min(L, pos + periods[k][1]); ++i) q[(size_t)i] = 0;
                    pos += periods[k][1];
                }
                if (rep == 2) for (auto &x : q) if (g_rng() % 50 == 0) x ^= 1;
                check(q, ws, gt, "period");
            }
        // all zero, all one, and the lengths around the window, around 1024 and around 2048 (random, zero and one)
        for (int L : {ws - 1, ws, ws + 1, 1023, 1024, 1025, 2047, 2048, 2049, ws + 31, ws + 32, ws + 33, ws + 64 * 32, ws + 64 * 32 + 1, 70000})
            for (int fill = 0; fill < 4; ++fill) {
                if (L < 1) continue;
                std::vector<uint8_t> q((size_t)L);
                for (auto &x : q) x = fill == 0 ? 0 : fill == 1 ? 1 : fill == 2 ? (uint8_t)(g_rng() & 1) : (uint8_t)(g_rng() % 10 != 0);
                check(q, ws, gt, "length");
            }
        // random: densities, runs, a clean read with holes, covered only at its two ends
        for (int rep = 0; rep < n_random; ++rep) {
            const int L = ws + 1 + (int)(g_rng() % 40000);
            std::vector<uint8_t> q((size_t)L);
            const int style = rep % 5;
            if (style == 0) { const int p = (int)(g_rng() % 101); for (auto &x : q) x = (int)(g_rng() % 100) < p; }
            else if (style == 1) { int run = 0, v = 1; for (auto &x : q) { if (run-- <= 0) { v ^= 1; run = (int)(g_rng() % (uint64_t)(2 * ws + 2)); } x = (uint8_t)v; } }
            else if (style == 2) { for (auto &x : q) x = 1; for (int z = 0; z < 8; ++z) { const int a = (int)(g_rng() % (uint64_t)L); for (int i = a; i < std::min(L, a + (int)(g_rng() % 5000)); ++i) q[(size_t)i] = 0; } }
            else if (style == 3) { const int p = 45 + (int)(g_rng() % 10); int run = 0, v = 0; for (auto &x : q) { if (run-- <= 0) { v = (int)(g_rng() % 100) < p; run = (int)(g_rng() % 40); } x = (uint8_t)v; } }
            else { for (auto &x : q) x = 0; for (int i = 0; i < std::min(16, L); ++i) q[(size_t)i] = q[(size_t)(L - 1 - i)] = 1; }
            check(q, ws, gt, "random");
        }
        printf("ws %d (%s): %ld words, %ld replayed\n", ws, pays ? "the grid pays" : "no paying regime", g_words - words0, g_replayed - rep0);
    }
    printf("exactness: %ld cases, %ld mismatches\n", g_cases, g_bad);
    return g_bad != 0;
}
