// summary_select_host.cpp — the host side of flx_summary's radix selection (filtlong_amd/csrc/summary_select.h) driven through its
// four passes with histograms computed here, the way the kernel computes them (an entry adds (1, length) to the row of its prefix,
// if that prefix is still alive), and all ten targets — N10 .. N90 and the median — compared with a sort.  Random and engineered
// length sets, each as 1, 2 and 3 "ranks": the entries are dealt to the ranks (unevenly, one share empty), every rank builds its own
// histograms and they are summed bin by bin before the step.  Built with -fsanitize=address,undefined by tests/test_summary_host.py.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "../filtlong_amd/csrc/summary_select.h"

namespace sel = flx_summary_select;

struct Want {
    int32_t nx[9], median;
};

static Want by_sort(std::vector<int32_t> v) {
    Want w{};
    if (v.empty()) return w;
    std::stable_sort(v.begin(), v.end(), [](int32_t a, int32_t b) { return a > b; });
    unsigned __int128 bases = 0;
    for (int32_t x : v) bases += (uint32_t)x;
    w.median = v[v.size() - 1 - (v.size() - 1) / 2];  // entry (n - 1) / 2 of the ascending order
    for (int t = 0; t < 9; ++t) {
        if (bases == 0) continue;
        unsigned __int128 cum = 0;
        for (int32_t x : v) {
            cum += (uint32_t)x;
            if (100 * cum >= (unsigned __int128)(10 * (t + 1)) * bases) {
                w.nx[t] = x;
                break;
            }
        }
    }
    return w;
}

// what k_summary_select leaves for one rank's entries
static void rows_of(const sel::State &s, const std::vector<int32_t> &v, std::vector<sel::Bin> &rows) {
    const int shift = sel::shift_of(s);
    for (int32_t len : v) {
        const uint32_t key = (uint32_t)len;
        const uint32_t pre = (uint32_t)((uint64_t)key >> (shift + 8));
        for (int r = 0; r < s.n_rows; ++r)
            if (s.row_prefix[r] == pre) {
                sel::Bin &b = rows[(size_t)r * sel::kDigits + ((key >> shift) & 255u)];
                b.count += 1;
                b.bases += key;
            }
    }
}

static long g_cases = 0, g_bad = 0, g_shared_rows = 0;

static void check(const char *what, const std::vector<int32_t> &v, int ranks) {
    // uneven shares, rank 1 (of 3) empty
    std::vector<std::vector<int32_t>> share((size_t)ranks);
    for (size_t i = 0; i < v.size(); ++i) {
        size_t r = 0;
        if (ranks == 2) r = i % 3 == 0 ? 1 : 0;
        if (ranks == 3) r = i % 4 == 0 ? 2 : 0;
        share[r].push_back(v[i]);
    }
    uint64_t n = 0, bases = 0;
    for (auto &sh : share)
        for (int32_t x : sh) ++n, bases += (uint32_t)x;
    sel::State s;
    sel::init(s, n, bases);
    while (s.pass < sel::kPasses) {
        if (s.n_rows < 1 || s.n_rows > sel::kTargets) { printf("FAIL %s: %d rows\n", what, s.n_rows); ++g_bad; return; }
        if (s.n_rows < sel::kTargets) ++g_shared_rows;
        std::vector<sel::Bin> sum((size_t)s.n_rows * sel::kDigits, sel::Bin{0, 0});
        for (auto &sh : share) {
            std::vector<sel::Bin> rows((size_t)s.n_rows * sel::kDigits, sel::Bin{0, 0});
            rows_of(s, sh, rows);
            for (size_t k = 0; k < sum.size(); ++k) sum[k].count += rows[k].count, sum[k].bases += rows[k].bases;
        }
        sel::step(s, sum.data());
    }
    const Want w = by_sort(v);
    ++g_cases;
    bool ok = s.consistent && sel::value(s, sel::kMedian) == w.median;
    for (int t = 0; t < 9; ++t) ok = ok && sel::value(s, t) == w.nx[t];
    if (!ok) {
        ++g_bad;
        printf("FAIL %s (n %llu, %d ranks): median %d want %d;", what, (unsigned long long)n, ranks, sel::value(s, sel::kMedian), w.median);
        for (int t = 0; t < 9; ++t) printf(" N%d %d want %d", 10 * (t + 1), sel::value(s, t), w.nx[t]);
        printf("\n");
    }
}

static void check_all(const char *what, const std::vector<int32_t> &v) {
    for (int ranks = 1; ranks <= 3; ++ranks) check(what, v, ranks);
}

int main(int argc, char **argv) {
    const int n_random = argc > 1 ? atoi(argv[1]) : 200;
    const int32_t kMax = 0x7fffffff;
    check_all("empty", {});
    check_all("one entry", {12345});
    check_all("one entry of 0", {0});
    check_all("one entry of 2^31-1", {kMax});
    check_all("every entry 0", std::vector<int32_t>(1000, 0));
    check_all("all equal", std::vector<int32_t>(777, 4242));
    check_all("all equal, 2^31-1", std::vector<int32_t>(5, kMax));
    check_all("three of 2^31-1 (bases > 2^32)", {kMax, kMax, kMax});
    check_all("two entries", {5, 7});
    check_all("two equal entries", {7, 7});
    {
        std::vector<int32_t> v;
        for (int i = 0; i < 256; ++i) v.push_back(0x12345600 + i);  // only the lowest byte differs
        check_all("lowest byte only", v);
        for (int i = 0; i < 300; ++i) v.push_back(0x12345600 + (i * 7) % 256);
        check_all("lowest byte only, repeats", v);
    }
    {
        std::vector<int32_t> v;
        for (int i = 0; i < 128; ++i) v.push_back((i << 24) | 0x00abcdef);  // only the highest byte differs
        check_all("highest byte only", v);
        check_all("top byte: two values", {0x01000000, 0x7f000000, 0x01000000, 0x7f000000, 0x01000000});
        check_all("bottom byte: two values", {0x00345601, 0x003456fe, 0x00345601, 0x003456fe, 0x00345601});
    }
    {
        std::vector<int32_t> v;  // zeros beside a few long entries: the Nx never stop at an entry of length 0
        for (int i = 0; i < 500; ++i) v.push_back(0);
        v.push_back(10); v.push_back(1); v.push_back(1);
        check_all("zeros and a few", v);
    }
    {
        std::vector<int32_t> v;  // every power of two and its neighbours
        for (int b = 0; b < 31; ++b) for (int d = -1; d <= 1; ++d) { const int64_t x = (1ll << b) + d; if (x >= 0 && x <= kMax) v.push_back((int32_t)x); }
        check_all("powers of two", v);
    }
    {
        // totals above 2^57: 2^27 entries of 2^31 - 1 would take too long to sort, so the histograms stand for them — the step
        // itself is what carries 100 * cum beyond 64 bits.  One row, all passes; the answer is 2^31 - 1 for every target.
        for (uint64_t n : {(uint64_t)1 << 27, (uint64_t)1 << 32, ((uint64_t)1 << 33) - 1}) {
            sel::State s;
            const uint64_t bases = n * (uint64_t)kMax;  // < 2^64
            sel::init(s, n, bases);
            while (s.pass < sel::kPasses) {
                std::vector<sel::Bin> rows((size_t)s.n_rows * sel::kDigits, sel::Bin{0, 0});
                const int shift = sel::shift_of(s);
                rows[((uint32_t)kMax >> shift) & 255u] = sel::Bin{n, bases};
                sel::step(s, rows.data());
            }
            ++g_cases;
            bool ok = s.consistent && s.n_rows == 1;
            for (int t = 0; t < sel::kTargets; ++t) ok = ok && sel::value(s, t) == kMax;
            if (!ok) { ++g_bad; printf("FAIL total %llu bases\n", (unsigned long long)bases); }
        }
        // ... and two lengths whose totals straddle 2^57: 3 * 2^26 entries of 2^31 - 1 above 2^27 entries of 2^30
        const uint64_t na = (uint64_t)3 << 26, nb = (uint64_t)1 << 27;
        const uint32_t la = (uint32_t)kMax, lb = 1u << 30;
        const uint64_t bases = na * la + nb * lb;
        sel::State s;
        sel::init(s, na + nb, bases);
        while (s.pass < sel::kPasses) {
            std::vector<sel::Bin> rows((size_t)s.n_rows * sel::kDigits, sel::Bin{0, 0});
            const int shift = sel::shift_of(s);
            for (int r = 0; r < s.n_rows; ++r) {
                if ((uint32_t)((uint64_t)la >> (shift + 8)) == s.row_prefix[r]) { auto &b = rows[(size_t)r * 256 + ((la >> shift) & 255u)]; b.count += na; b.bases += na * la; }
                if ((uint32_t)((uint64_t)lb >> (shift + 8)) == s.row_prefix[r]) { auto &b = rows[(size_t)r * 256 + ((lb >> shift) & 255u)]; b.count += nb; b.bases += nb * lb; }
            }
            sel::step(s, rows.data());
        }
        ++g_cases;
        bool ok = s.consistent;
        for (int t = 0; t < 9; ++t) {  // N(x) is the long length while x * bases <= 100 * na * la
            const bool in_a = (unsigned __int128)100 * na * la >= (unsigned __int128)(10 * (t + 1)) * bases;
            ok = ok && sel::value(s, t) == (int32_t)(in_a ? la : lb);
        }
        ok = ok && sel::value(s, sel::kMedian) == (int32_t)la;  // descending entry (na + nb) / 2 = 5 * 2^25 < na
        if (!ok) { ++g_bad; printf("FAIL two lengths around 2^57\n"); }
    }
    std::mt19937_64 rng(20240607);
    for (int c = 0; c < n_random; ++c) {
        const int kind = c % 5;
        const size_t n = 1 + rng() % (kind == 4 ? 5000 : 600);
        std::vector<int32_t> v(n);
        for (auto &x : v) {
            if (kind == 0) x = (int32_t)(rng() & 0x7fffffff);                      // anything
            else if (kind == 1) x = (int32_t)(rng() % 60000);                      // read-like
            else if (kind == 2) x = (int32_t)((rng() % 3) << 24 | (rng() % 4));    // few distinct values: shared rows
            else if (kind == 3) x = (int32_t)(0x7fffff00u + rng() % 256);          // the top of the range: bases > 2^32
            else x = (int32_t)(1000 + rng() % 16);                                 // many ties
        }
        check_all("random", v);
    }
    printf("select: %ld cases, %ld mismatches, %ld passes with shared rows\n", g_cases, g_bad, g_shared_rows);
    return g_bad ? 1 : 0;
}
