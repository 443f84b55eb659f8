// adapters.h — --trim_adapters: known adapters are cut off the two ends of every read.  The host core of adapters.hip, and like
// qsplit.h / screen.h plain C++ that a HIP kernel and a host program both include.  The reference has no counterpart: its users run
// an adapter trimmer over the whole file in front of it.
//
// Everything is defined on integers, so any decomposition (lanes, waves, workgroups, chunks, ranks) gives the same answer.
//   patterns      every sequence of the adapter file, upper-cased, and its reverse complement: pattern 2 i is sequence i, pattern
//                 2 i + 1 its reverse complement.  A sequence has 12 to 64 bases of ACGT; at most 128 sequences.  A pattern of m
//                 bases may carry k = m * E / 100 edits (integer division), E = --adapter_errors, 0..40.
//   texts         W = --adapter_window, 1..1024; for a read of L bases n = min(L, W).  The head text is read[0, n).  The tail text
//                 is read[L - n, L) reversed and is matched against the patterns reversed: the tail is the head computation on the
//                 reversed read.  Lower case is folded; a text byte outside ACGTacgt equals no pattern base.
//   match         unit-cost edit distance of the whole pattern against any substring of the text: D[0][j] = 0, D[i][0] = i,
//                 d(j) = D[m][j] for 1 <= j <= n; dmin = min d(j), jbest the LARGEST j with d(j) = dmin.  The pattern hits iff
//                 n >= 1 and dmin <= k.
//   cut           per end, key = max over the hitting patterns of (jbest << 8) | pattern, 0 without a hit; cut = key >> 8.
//                 s = cut_head, e = L - cut_tail.  No hit at either end: no child, first = 0, last = L.  s < e: one child [s, e).
//                 s >= e: no child, first = last = -1 — the read stays one failing entry, like a wholly bad read of qsplit.h.
//
// The column walk is Myers' bit-vector form (J. ACM 46, 1999; the search variant, whose row 0 is all zero): m <= 64 is one word, bit
// m - 1 of the horizontal deltas carries the change of D[m][j].  Bits above m - 1 hold whatever: carries only travel upwards.
#pragma once

#include <stdint.h>

#include <vector>

#if defined(__HIPCC__)
#define ADAPTERS_FN __host__ __device__ __forceinline__
#else
#define ADAPTERS_FN inline
#endif

namespace adapters {

constexpr int kMinBases = 12, kMaxBases = 64;  // of one sequence
constexpr int kMaxSeqs = 128;                  // 256 patterns: the pattern index is the low byte of a key
constexpr int kMaxErrors = 40;                 // E, percent
constexpr int kMaxWindow = 1024;               // W
constexpr uint32_t kNoBase = 4;                // the code of a text byte outside ACGTacgt

ADAPTERS_FN bool is_acgt(uint8_t c) {
    const uint32_t d = (uint32_t)(c | 0x20u) - 0x61u;  // a 0, c 2, g 6, t 19
    return d < 32u && ((0x80045u >> d) & 1u);
}
// A 0, C 1, G 2, T 3 in either case, kNoBase for any other byte
ADAPTERS_FN uint32_t code_of(uint8_t c) { return is_acgt(c) ? (((uint32_t)c >> 1) ^ ((uint32_t)c >> 2)) & 3u : kNoBase; }

// One pattern as the kernel reads it: bit i of peq_head[c] says base i is c, bit i of peq_tail[c] says base m - 1 - i is c.
struct Pattern {
    uint64_t peq_head[4];
    uint64_t peq_tail[4];
    uint32_t m, k;
};

ADAPTERS_FN uint32_t edits_allowed(uint32_t m, uint32_t errors_percent) { return m * errors_percent / 100u; }

// the column state of one (text, pattern) pair
struct Column {
    uint64_t pv, mv;
    int32_t score;  // D[m][j]
    int32_t dmin, jbest;
};

ADAPTERS_FN void column_start(Column *s, uint32_t m) {
    s->pv = ~0ull;
    s->mv = 0;
    s->score = (int32_t)m;
    s->dmin = 0x7fffffff;
    s->jbest = 0;
}

// text base j (1-based) whose match mask against the pattern is eq; top = 1 << (m - 1)
ADAPTERS_FN void column_step(Column *s, uint64_t eq, uint64_t top, int32_t j) {
    const uint64_t pv = s->pv, mv = s->mv;
    const uint64_t xv = eq | mv;
    const uint64_t xh = (((eq & pv) + pv) ^ pv) | eq;
    uint64_t ph = mv | ~(xh | pv);
    uint64_t mh = pv & xh;
    s->score += (ph & top) ? 1 : 0;
    s->score -= (mh & top) ? 1 : 0;
    ph <<= 1;  // (row 0 is all zero: nothing comes in at the bottom)
    mh <<= 1;
    s->pv = mh | ~(xv | ph);
    s->mv = ph & xv;
    if (s->score <= s->dmin) {  // <=: the largest j wins a tie
        s->dmin = s->score;
        s->jbest = j;
    }
}

ADAPTERS_FN uint64_t select_eq(const uint64_t peq[4], uint32_t code) {
    uint64_t eq = 0;
    eq = code == 0u ? peq[0] : eq;
    eq = code == 1u ? peq[1] : eq;
    eq = code == 2u ? peq[2] : eq;
    eq = code == 3u ? peq[3] : eq;
    return eq;
}

// The child rule: from the two keys of a read of L bases its number of children (0 or 1), the child [*start, *end), first and last.
ADAPTERS_FN int child_of(uint32_t key_head, uint32_t key_tail, int64_t L, int32_t *first, int32_t *last) {
    if ((key_head | key_tail) == 0u) {
        *first = 0;
        *last = (int32_t)L;
        return 0;
    }
    const int64_t s = (int64_t)(key_head >> 8), e = L - (int64_t)(key_tail >> 8);
    if (s < e) {
        *first = (int32_t)s;
        *last = (int32_t)e;
        return 1;
    }
    *first = -1;
    *last = -1;
    return 0;
}

// ---- host only from here --------------------------------------------------------------------------------------------------------

inline uint8_t complement(uint8_t c) { return c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : 'A'; }

inline void reverse_complement(const uint8_t *in, uint32_t m, uint8_t *out) {
    for (uint32_t i = 0; i < m; ++i) out[i] = complement(in[m - 1 - i]);
}

// the pattern of m upper-case bases of ACGT
inline Pattern make_pattern(const uint8_t *bases, uint32_t m, uint32_t errors_percent) {
    Pattern p = {};
    p.m = m;
    p.k = edits_allowed(m, errors_percent);
    for (uint32_t i = 0; i < m; ++i) {
        p.peq_head[code_of(bases[i])] |= 1ull << i;
        p.peq_tail[code_of(bases[m - 1 - i])] |= 1ull << i;
    }
    return p;
}

// The patterns of the sequences bases[offsets[i] .. offsets[i] + lengths[i]).  0: fine; 1 + i: sequence i is outside 12..64 bases
// or not ACGTacgt; -1: too many sequences, E or W out of range.
inline int64_t build(const uint8_t *bases, const uint64_t *offsets, const int64_t *lengths, uint64_t n_seqs, int errors_percent, int window,
                     std::vector<Pattern> *out) {
    out->clear();
    if (n_seqs > (uint64_t)kMaxSeqs || errors_percent < 0 || errors_percent > kMaxErrors || window < 1 || window > kMaxWindow) return -1;
    for (uint64_t s = 0; s < n_seqs; ++s) {
        const int64_t m = lengths[s];
        if (m < kMinBases || m > kMaxBases) return 1 + (int64_t)s;
        uint8_t fwd[kMaxBases], rev[kMaxBases];
        for (int64_t i = 0; i < m; ++i) {
            const uint8_t c = bases[offsets[s] + (uint64_t)i];
            if (!is_acgt(c)) return 1 + (int64_t)s;
            fwd[i] = (uint8_t)(c & ~0x20u);
        }
        reverse_complement(fwd, (uint32_t)m, rev);
        out->push_back(make_pattern(fwd, (uint32_t)m, (uint32_t)errors_percent));
        out->push_back(make_pattern(rev, (uint32_t)m, (uint32_t)errors_percent));
    }
    return 0;
}

// The serial walk for one end of one read: the kernel's oracle.  side 0: the head, 1: the tail.  Reads read[0, L) and nothing else.
inline uint32_t end_key(const uint8_t *read, int64_t L, int side, int64_t W, const Pattern *patterns, uint32_t n_patterns) {
    const int64_t n = L < W ? L : W;
    uint32_t key = 0;
    for (uint32_t p = 0; p < n_patterns; ++p) {
        const Pattern &pat = patterns[p];
        const uint64_t *peq = side ? pat.peq_tail : pat.peq_head;
        const uint64_t top = 1ull << (pat.m - 1);
        Column col;
        column_start(&col, pat.m);
        for (int64_t j = 0; j < n; ++j) {
            const uint8_t c = side ? read[L - 1 - j] : read[j];
            column_step(&col, select_eq(peq, code_of(c)), top, (int32_t)(j + 1));
        }
        if (n >= 1 && col.dmin <= (int32_t)pat.k) {
            const uint32_t mine = ((uint32_t)col.jbest << 8) | p;
            if (mine > key) key = mine;
        }
    }
    return key;
}

}  // namespace adapters
