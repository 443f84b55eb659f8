// sim_cover_segments.cpp — the segment arithmetic of the coverage stage's cooperative path (filtlong_amd/csrc/cover_segments.h,
// the very header the kernels and the host use) held against the definition of coverage on the host.
//
// Coverage (src/read.cpp:43-58): a rolling 2-bit 16-mer (C/c 1, G/g 2, T/t 3, anything else 0), one set lookup per position from the
// 16th base on, bases i-15..i marked on a hit.  For byte streams against a random member set this program computes
//   (a) the coverage of the whole read, brute force: bits, covered count, first and last covered base as the cover kernels give
//       them (first = index of the first covered base, last = index of the last one + 1, both -1 without coverage), and
//   (b) the same stitched from segments: every segment's virtual read [S, T) is covered AS A READ OF ITS OWN (nothing outside it is
//       looked at), restricted to its emit range, its bits written at S + the virtual position, its count / first / last added with
//       flx_cover_seg_add
// and compares them bit for bit — for every length from 0 to max_len (first argument, default 3000) and segment sizes of 32, 64, 96,
// 128, 1024 and 2048 bases in place of the kernels' P x 1024.  Streams: random bases over a set dense enough that islands and
// gaps of every length occur, random bases over a sparse set, a member island of 16 .. 64 bases moved across every position near
// the first and the last segment boundary, fully covered reads, reads without coverage, reads covered only in their first and
// last 16 bases.
//   g++ -O2 -std=c++17 -o sim_cover_segments tools/sim_cover_segments.cpp && ./sim_cover_segments [max_len]
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <unordered_set>
#include <vector>

#include "../filtlong_amd/csrc/cover_segments.h"

static inline uint32_t code(uint8_t c) {
    switch (c) {
        case 'C': case 'c': return 1;
        case 'G': case 'g': return 2;
        case 'T': case 't': return 3;
        default: return 0;
    }
}

struct Cover {
    std::vector<uint8_t> bits;  // one per base
    int count = 0, first = -1, last = -1;
};

// the definition, on bases [from, to) of `seq` taken as a read of their own; bits land at out.bits[at + i] for the bases inside
// [emit_lo, emit_hi) of that read, totals are of those bases only, in that read's coordinates
static void cover_read(const std::vector<uint8_t> &seq, int from, int to, const std::unordered_set<uint32_t> &set, int emit_lo, int emit_hi,
                       std::vector<uint8_t> &bits_out, int at, int *count, int *first, int *last) {
    const int L = to - from;
    std::vector<uint8_t> cov((size_t)L, 0);
    uint32_t k = 0;
    for (int i = 0; i < L; ++i) {
        k = (k << 2) | code(seq[(size_t)(from + i)]);
        if (i >= 15 && set.count(k))
            for (int j = i - 15; j <= i; ++j) cov[(size_t)j] = 1;
    }
    int c = 0, f = -1, l = -1;
    for (int i = emit_lo; i < emit_hi; ++i) {
        if (bits_out[(size_t)(at + i)] != 2) {  // a base two segments write: the stitched plane would depend on the order
            fprintf(stderr, "base %d written twice\n", at + i);
            exit(2);
        }
        bits_out[(size_t)(at + i)] = cov[(size_t)i];
        if (cov[(size_t)i]) {
            ++c;
            if (f < 0) f = i;
            l = i + 1;
        }
    }
    *count = c;
    *first = f;
    *last = l;
}

static long long g_cases = 0, g_mismatches = 0, g_segments = 0;

static void check(const std::vector<uint8_t> &seq, const std::unordered_set<uint32_t> &set, int seg_bases, const char *what) {
    const int L = (int)seq.size();
    Cover whole;
    whole.bits.assign((size_t)L, 2);
    cover_read(seq, 0, L, set, 0, L, whole.bits, 0, &whole.count, &whole.first, &whole.last);
    Cover st;
    st.bits.assign((size_t)L, 2);
    CoverTotals tot = {0, -1, -1};
    const long long n_seg = flx_cover_seg_count(L, seg_bases);
    bool bad = false;
    long long owned = 0;
    for (long long k = 0; k < n_seg; ++k) {
        const CoverSeg s = flx_cover_seg(L, seg_bases, k);
        // what the kernels rely on: S on a 32-base boundary, the emit range inside the virtual read, on 32-base boundaries except
        // at the read's end, never empty, with 15 bases of context wherever the read has them
        if (s.S % 32 != 0 || s.S < 0 || s.T > L || s.emit_lo < 0 || s.emit_hi > s.T - s.S || s.emit_lo >= s.emit_hi || s.emit_lo % 32 != 0 ||
            (s.emit_hi % 32 != 0 && s.S + s.emit_hi != L) || (s.S > 0 && s.emit_lo < 15) || (s.T < L && (s.T - s.S) - s.emit_hi < 15))
            bad = true;
        owned += s.emit_hi - s.emit_lo;
        int c, f, l;
        cover_read(seq, s.S, s.T, set, s.emit_lo, s.emit_hi, st.bits, s.S, &c, &f, &l);
        flx_cover_seg_add(tot, s.S, c, f, l);
        ++g_segments;
    }
    if (owned != L) bad = true;
    ++g_cases;
    if (bad || st.bits != whole.bits || tot.count != whole.count || tot.first != whole.first || tot.last != whole.last) {
        ++g_mismatches;
        if (g_mismatches <= 10)
            fprintf(stderr, "MISMATCH %s: L %d, segment %d: count %d / %d, first %d / %d, last %d / %d%s\n", what, L, seg_bases, tot.count, whole.count,
                    tot.first, whole.first, tot.last, whole.last, bad ? " (segment bounds)" : "");
    }
}

int main(int argc, char **argv) {
    const int max_len = argc > 1 ? atoi(argv[1]) : 3000;
    std::mt19937_64 rng(20240611);
    const char acgt[4] = {'A', 'C', 'G', 'T'};
    auto random_bases = [&](int n) {
        std::vector<uint8_t> s((size_t)n);
        for (auto &c : s) c = (uint8_t)acgt[rng() & 3];
        return s;
    };
    // a member text: its 16-mers are the sparse set; the dense set also holds a fifth of all 16-mers of a stream drawn over C and G
    // only (2^16 of them), so that random C/G streams are covered in islands and gaps of every length
    const std::vector<uint8_t> text = random_bases(20000);
    std::unordered_set<uint32_t> sparse;
    {
        uint32_t k = 0;
        for (size_t i = 0; i < text.size(); ++i) {
            k = (k << 2) | code(text[i]);
            if (i >= 15) sparse.insert(k);
        }
    }
    std::unordered_set<uint32_t> dense = sparse;
    for (uint32_t v = 0; v < (1u << 16); ++v) {
        if (rng() % 5) continue;
        uint32_t k = 0;
        for (int b = 0; b < 16; ++b) k = (k << 2) | (((v >> b) & 1u) ? 1u : 2u);
        dense.insert(k);
    }
    auto cg_bases = [&](int n) {
        std::vector<uint8_t> s((size_t)n);
        for (auto &c : s) c = (rng() & 1) ? 'C' : 'G';
        return s;
    };
    auto low = [&](int n) {  // no member 16-mer ("ACG" repeated; checked below)
        std::vector<uint8_t> s((size_t)n);
        for (int i = 0; i < n; ++i) s[(size_t)i] = (uint8_t)"ACG"[i % 3];
        return s;
    };
    {
        const std::vector<uint8_t> l = low(64);
        uint32_t k = 0;
        for (size_t i = 0; i < l.size(); ++i) {
            k = (k << 2) | code(l[i]);
            if (i >= 15 && dense.count(k)) {
                fprintf(stderr, "the background holds a member\n");
                return 2;
            }
        }
    }
    const int seg_sizes[] = {32, 64, 96, 128, 1024, 2048};
    for (int seg : seg_sizes) {
        for (int L = 0; L <= max_len; ++L) {
            check(cg_bases(L), dense, seg, "islands and gaps");
            if (L % 7 == 0) {
                std::vector<uint8_t> s = random_bases(L);  // pieces of the text between junk, other letters in places
                for (int p = 0; p + 40 < L; p += 40 + (int)(rng() % 300)) {
                    const int n = std::min(L - p, 16 + (int)(rng() % 200));
                    const size_t from = (size_t)(rng() % (text.size() - (size_t)n));
                    memcpy(&s[(size_t)p], &text[from], (size_t)n);
                    if (rng() % 3 == 0) s[(size_t)(p + n / 2)] = 'N';
                }
                check(s, sparse, seg, "text pieces");
            }
        }
        // engineered: fully covered, no coverage, first and last 16 bases only; an island across the first and the last boundary
        for (int r : {0, 1, 15, 16, 17, 31, 32, 33, seg - 1}) {
            const int L = 4 * seg + r;
            if (L <= (int)text.size()) check(std::vector<uint8_t>(text.begin() + 100, text.begin() + 100 + L), sparse, seg, "fully covered");
            check(low(L), sparse, seg, "no coverage");
            if (L >= 32) {
                std::vector<uint8_t> s = low(L);
                memcpy(&s[0], &text[500], 16);
                memcpy(&s[(size_t)(L - 16)], &text[700], 16);
                check(s, sparse, seg, "first and last 16 bases");
            }
            const int last_boundary = (int)(flx_cover_seg_count(L, seg) - 1) * seg;
            for (int boundary : {seg, last_boundary})
                for (int island : {16, 17, 31, 32, 33, 48, 64})
                    for (int d = -70; d <= 40; ++d) {
                        const int at = boundary + d;
                        if (at < 0 || at + island > L) continue;
                        std::vector<uint8_t> s = low(L);
                        memcpy(&s[(size_t)at], &text[1000 + (size_t)(rng() % 5000)], (size_t)island);
                        check(s, sparse, seg, "island");
                    }
        }
    }
    printf("exactness: %lld cases, %lld segments, %lld mismatches\n", g_cases, g_segments, g_mismatches);
    return g_mismatches ? 1 : 0;
}
