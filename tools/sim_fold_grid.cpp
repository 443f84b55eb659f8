// sim_fold_grid.cpp — the integer-grid window fold, on the host: the grid table and the start of a regime are the
// kernels' own code (filtlong_amd/csrc/fold_grid_tab.h), the walk over the words is restated here.
//
// Reference semantics: src/read.cpp:216-236 with qualities 0.0 / 1.0:  w0 = cnt / ws;  per step  w -= q[j-ws]/ws; w += q[j]/ws;
// mn = min(mn, w).  Claim: while w stays inside a GROUP of binades in which fl(1/ws) rounds to the same real number d* on every
// binade's grid (no ties), and does not reach a binade above the highest one it has been in since the regime began, every step is
// exact:  w = w_b + (c - c_b) * d*  — so a word of 32 positions is (total, min prefix, max prefix) of the +-1 walk of its bits.
// Everything else (a new record-high binade, leaving the group, ties, w = 0) replays the word in floating point.
//   (1) exactness: random bit streams x many window sizes, the regime fold against the plain FP fold, bit for bit;
//   (2) how often a wave of 64 lanes has to take the slow path on C3-like coverage (substitution rates 0..12 %, junk blocks).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../filtlong_amd/csrc/fold_grid_tab.h"

// The table (build_grid_table) and the start of a regime (grid_regime_begin) are the kernels' own: fold_grid_tab.h.  A window size
// without a table (ws < 8) has no regime anywhere and folds in plain floating point, as the kernel does.
static long g_reason[4];  // slow words by reason: 0 no regime, 1 below, 2 above
static int g_nibble = 0;    // 1: a slow word is replayed from its first nibble that leaves the regime (costed in round 6, NOT built: below); 0: whole, what the kernel does
static long g_fp_steps = 0; // positions replayed in floating point
static int g_ctz_rule = 1;  // the top of a regime: the highest binade on whose grid w_b already lies (0: the binade w_b is in, passed as `top`)

struct Fold { double w, mn; };
// plain FP fold of positions [ws, L) given bits
static Fold fold_fp(const std::vector<uint8_t> &q, int ws) {
    const int L = (int)q.size();
    volatile double one = 1.0, wsd = (double)ws;
    const double d = one / wsd;
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

// regime fold; `slow` gets the word indices that took the FP path
static Fold fold_grid(const std::vector<uint8_t> &q, int ws, const GridTab &t, std::vector<int> *slow) {
    const int L = (int)q.size();
    volatile double one = 1.0, wsd = (double)ws;
    const double d = one / wsd;
    long cnt = 0;
    for (int i = 0; i < ws; ++i) cnt += q[i];
    double w = (double)cnt / wsd, mn = w;
    int j = ws;
    // words aligned to 32 from the first multiple of 32 >= ws, like the kernel (the head runs bit by bit)
    for (; j < L && (j & 31); ++j) {
        w -= q[j - ws] ? d : 0.0;
        w += q[j] ? d : 0.0;
        if (w < mn) mn = w;
    }
    GridRegime r = grid_regime_begin(t, w, (double)ws, !g_ctz_rule);
    int c = 0, cmin = 0;
    auto flush = [&]() {
        if (r.ds > 0.0) {
            const double wn = grid_value(r, c);
            const double m2 = grid_value(r, cmin);
            if (m2 < mn) mn = m2;
            w = wn;
        }
    };
    for (; j + 32 <= L; j += 32) {
        int tt = 0, mp = 0, xp = 0;
        bool any = false;
        for (int i = 0; i < 32; ++i) {
            const int x = (int)q[j + i] - (int)q[j + i - ws];
            any = any || q[j + i] || q[j + i - ws];
            tt += x;
            mp = std::min(mp, tt);
            xp = std::max(xp, tt);
        }
        if (!any) continue;  // (0,0) steps change nothing in any regime
        if (r.ds > 0.0 && c + mp >= r.lo && c + xp <= r.hi) {
            cmin = std::min(cmin, c + mp);
            c += tt;
            continue;
        }
        // Round 6, costed and NOT built (g_nibble = 1 runs it here): replay a slow word only from the first NIBBLE (4 positions: the
        // granularity of the kernel's walk table) whose prefix leaves the regime — the steps in front of it are still exact on the grid, the
        // same criterion on a shorter walk.  Exact (the cases below run both forms), but 26 of the 32 positions are still replayed on the
        // C3-like reads (half the slow words have no regime at all — w in the tie binade or at 0 — and start at position 0), and finding the
        // nibble costs the kernel a second walk through the table: a loss.
        int first = 0;  // first position replayed in floating point
        if (g_nibble && r.ds > 0.0) {
            int pre = 0, lo = 0, hi = 0;  // the walk through the nibbles that stay inside
            for (int k = 0; k < 8; ++k) {
                int p2 = pre, lo2 = lo, hi2 = hi;
                for (int i = 4 * k; i < 4 * k + 4; ++i) {
                    p2 += (int)q[j + i] - (int)q[j + i - ws];
                    lo2 = std::min(lo2, p2);
                    hi2 = std::max(hi2, p2);
                }
                if (!(c + lo2 >= r.lo && c + hi2 <= r.hi)) break;
                pre = p2; lo = lo2; hi = hi2;
                first = 4 * k + 4;
            }
            cmin = std::min(cmin, c + lo);
            c += pre;
        }
        g_fp_steps += 32 - first;
        flush();
        if (slow) slow->push_back(j >> 5);
        ++g_reason[!(r.ds > 0.0) ? 0 : (c + mp < r.lo ? 1 : 2)];
        for (int i = first; i < 32; ++i) {
            w -= q[j + i - ws] ? d : 0.0;
            w += q[j + i] ? d : 0.0;
            if (w < mn) mn = w;
        }
        r = grid_regime_begin(t, w, (double)ws, !g_ctz_rule);
        c = 0;
        cmin = 0;
    }
    flush();
    for (; j < L; ++j) {
        w -= q[j - ws] ? d : 0.0;
        w += q[j] ? d : 0.0;
        if (w < mn) mn = w;
    }
    return {w, mn};
}

static std::vector<uint8_t> c3_like(std::mt19937_64 &g, int L) {
    std::vector<uint8_t> sub((size_t)L, 0), cov((size_t)L, 0);
    const int erate = (int)(g() % 13);
    for (int i = 0; i < L; ++i) sub[i] = (int)(g() % 100) < erate && (g() & 3) != 0;  // (a substitution by the same base changes nothing)
    int js = -1, je = -1;
    if (L > 3000 && g() % 10 < 3) { js = 500 + (int)(g() % (uint64_t)(L - 2000)); je = std::min(js + 800, L); }
    for (int i = 0; i < L; ++i) if (i >= js && i < je) sub[i] = (g() & 3) != 0;
    int run = 0;
    for (int i = 0; i < L; ++i) {
        run = sub[i] ? 0 : run + 1;
        if (run >= 16) for (int k = i - 15; k <= i; ++k) cov[k] = 1;
    }
    return cov;
}

int main(int argc, char **argv) {
    std::mt19937_64 g(12345);
    // (1) exactness
    long cases = 0, bad = 0;
    const int n_ws = argc > 1 ? atoi(argv[1]) : 400;
    for (int k = 0; k < n_ws; ++k) {
        const int ws = k < 40 ? (int[]){250, 100, 1, 2, 3, 5, 7, 16, 32, 33, 64, 127, 128, 129, 255, 256, 257, 500, 512, 1000, 1024, 2047, 2048, 4096, 9999, 10000, 31, 63, 65, 96, 97, 200, 300, 333, 400, 600, 750, 800, 900, 1500}[k] : 1 + (int)(g() % 3000);
        GridTab t;
        build_grid_table(ws, t);
        for (int rep = 0; rep < 30; ++rep) {
            const int L = ws + 64 + (int)(g() % 20000);
            std::vector<uint8_t> q((size_t)L);
            const int style = rep % 6;
            if (style == 0) q = c3_like(g, L);
            else if (style == 1) { const int p = (int)(g() % 100); for (auto &x : q) x = (int)(g() % 100) < p; }
            else if (style == 2) { int run = 0, v = 1; for (auto &x : q) { if (run-- <= 0) { v ^= 1; run = (int)(g() % (uint64_t)(2 * ws + 2)); } x = (uint8_t)v; } }
            else if (style == 3) { for (int i = 0; i < L; ++i) q[i] = (i / (1 + rep)) & 1; }
            else if (style == 4) { const int p = 45 + (int)(g() % 10); int run = 0, v = 0; for (auto &x : q) { if (run-- <= 0) { v = (int)(g() % 100) < p; run = (int)(g() % 40); } x = (uint8_t)v; } }
            else { for (auto &x : q) x = 1; for (int z = 0; z < 5; ++z) { const int a = (int)(g() % (uint64_t)L); for (int i = a; i < std::min(L, a + (int)(g() % 600)); ++i) q[i] = 0; } }
            const Fold a = fold_fp(q, ws);
            ++cases;
            for (int nib = 0; nib < 2; ++nib) {  // whole-word replay (the kernel) and replay from the first nibble outside (costed, not built)
                g_nibble = nib;
                const Fold b = fold_grid(q, ws, t, nullptr);
                if (memcmp(&a.w, &b.w, 8) || memcmp(&a.mn, &b.mn, 8)) {
                    if (++bad < 10) printf("MISMATCH ws %d style %d L %d nibble %d: w %a vs %a  mn %a vs %a\n", ws, style, L, nib, a.w, b.w, a.mn, b.mn);
                }
            }
            g_nibble = 0;
        }
    }
    printf("exactness: %ld cases, %ld mismatches\n", cases, bad);
    // the groups of the default window
    for (int ws : {250, 100, 1000, 500}) {
        GridTab t;
        build_grid_table(ws, t);
        printf("ws %d: groups", ws);  // a group begins behind a tie (d* = 0) or where top[] changes, and reaches up to its top[]
        for (int i = 0; i < t.n; ++i)
            if (t.dstar[i] != 0.0 && (i == 0 || t.dstar[i - 1] == 0.0 || t.top[i - 1] != t.top[i])) printf(" [2^%d, 2^%d)", t.e0 - 1023 + i, t.top[i] - 1023 + 1);
        printf("   ties at:");
        for (int i = 0; i < t.n; ++i) if (t.dstar[i] == 0.0) printf(" 2^%d", t.e0 - 1023 + i);
        printf("\n");
    }
    g_reason[0] = g_reason[1] = g_reason[2] = 0;
    g_fp_steps = 0;
    g_nibble = argc > 2 ? atoi(argv[2]) : 0;  // (second argument 1: the statistics of the nibble form)
    // (2) slow words per wave, C3-like reads (gamma lengths, sorted descending, 64 per wave)
    for (int rule = 0; rule < 2; ++rule)
    for (int ws : {250, 100, 500}) {
        g_ctz_rule = rule;
        printf("top of a regime %s: ", rule ? "by the grid w_b lies on" : "the binade w_b is in");
        GridTab t;
        build_grid_table(ws, t);
        const int n = 64 * 60;
        std::vector<int> len((size_t)n);
        std::gamma_distribution<double> gd(4.0, 2500.0);
        for (auto &x : len) x = std::max(ws + 100, std::min(200000, (int)gd(g)));
        std::sort(len.begin(), len.end(), std::greater<int>());
        long wave_words = 0, wave_slow = 0, lane_words = 0, lane_slow = 0;
        for (int w0 = 0; w0 < n; w0 += 64) {
            std::vector<std::vector<int>> slow(64);
            int maxw = 0;
            for (int l = 0; l < 64; ++l) {
                const std::vector<uint8_t> q = c3_like(g, len[(size_t)(w0 + l)]);
                fold_grid(q, ws, t, &slow[(size_t)l]);
                lane_slow += (long)slow[(size_t)l].size();
                lane_words += (len[(size_t)(w0 + l)] - ws) / 32;
                maxw = std::max(maxw, len[(size_t)(w0 + l)] / 32 + 1);
            }
            std::vector<char> any((size_t)maxw + 1, 0);
            for (auto &v : slow) for (int x : v) any[(size_t)x] = 1;
            for (char x : any) wave_slow += x;
            wave_words += (len[(size_t)w0] - ws) / 32;
        }
        printf("ws %d: lane-words %ld, slow %ld (%.3f %%); wave-words %ld, with a slow lane %ld (%.1f %%); reasons: no regime %ld, below %ld, above %ld; positions replayed per slow lane-word %.1f\n", ws, lane_words, lane_slow,
               100.0 * lane_slow / lane_words, wave_words, wave_slow, 100.0 * wave_slow / wave_words, g_reason[0], g_reason[1], g_reason[2], lane_slow ? (double)g_fp_steps / lane_slow : 0.0);
        g_fp_steps = 0;
        g_reason[0] = g_reason[1] = g_reason[2] = 0;
    }
    return bad != 0;
}
