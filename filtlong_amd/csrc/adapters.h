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
//   overhang      O = --adapter_overhang, 0..52 (kMaxBases - kMinBases), 0: off.  A read that begins or ends INSIDE an adapter pays
//                 one edit per missing base above; with O > 0 every (text, pattern) pair gets a second, ANCHORED walk.  Per pattern
//                 O_p = min(O, m - 12) (12 pattern bases always remain) and k'_p = (m - O_p) * E / 100: the allowance of the
//                 shortest truncated pattern, used for every truncation.  O_p = 0: no second walk.  The same texts, masks and
//                 recurrence with other borders: D[i][0] = max(0, i - O_p) (the first O_p pattern bases may be missing at no cost)
//                 and D[0][j] = j (the occurrence begins at the read's edge).  d'(j) = D[m][j], dmin' and jbest' as above; the
//                 walk hits iff n >= 1 and dmin' <= k'_p.  d'(j) >= j - m, so no j above m + k'_p can be a hit and a walk may stop
//                 after min(n, m + k'_p) columns.  At the tail the reversed pattern's first bases are the adapter's last: there
//                 the overhang frees the END of the adapter.
//   cut           per end, key = max over the hitting walks, free or anchored, of every pattern of (jbest << 8) | pattern, 0
//                 without a hit; cut = key >> 8.  (The key with overhang is never below the key without: the maximum only gains.)
//                 s = cut_head, e = L - cut_tail.  No hit at either end: no child, first = 0, last = L.  s < e: one child [s, e).
//                 s >= e: no child, first = last = -1 — the read stays one failing entry, like a wholly bad read of qsplit.h.
//
// --split_adapters: chimeras are split at the adapters INSIDE a read (adapters_split.hip).  The same patterns over the whole read.
//   hit ends      the text is the whole read, positions 1..L; pattern p of m bases may carry k2 = m * E2 / 100 edits, E2 =
//                 --adapter_split_errors, 0..40.  With the recurrence above d_p(j) = D[m][j]; j is a HIT END of p iff d_p(j) <= k2.
//   marks         every hit end (p, j) marks the bases [max(0, j - m), j); B is the union of all marks.  (Up to k2 bases more than
//                 the occurrence on either side: the price of a rule that needs no start position.)
//   children      [s, e) is what the ends rule leaves, unchanged.  No end hit and B empty: no child, first = 0, last = L.  Otherwise
//                 the children are the maximal runs of bases of [s, e) outside B, ascending; first is the first child's start, last
//                 the last child's end.  No base left: no child, first = last = -1.
//   pieces        A column started fresh (D[i][a'] = i) at text position a' computes the minimum over substrings that start at or
//                 behind a', so it never lies below the true d_p(j).  A substring within k2 edits of the pattern has at most m + k2
//                 bases, so for every j >= a' + m + k2 the fresh column gives d_p(j) <= k2 exactly when the true one does (values
//                 above k2 may differ and are never used).  k2 <= 40 % of m: the warm-up is at most 64 + 25 = 89 bases.  A piece
//                 [a, b) of a read is therefore settled by a walk from max(0, a - kWarmup) to b that reports only the hit ends j
//                 in (a, b]; its marks may reach back into the piece in front.
//
// The column walk is Myers' bit-vector form (J. ACM 46, 1999; the search variant, whose row 0 is all zero): m <= 64 is one word, bit
// m - 1 of the horizontal deltas carries the change of D[m][j].  Bits above m - 1 hold whatever: carries only travel upwards.
// The anchored walk is the same form with row 0 counting up: Pv = ~0 << O_p, Mv = 0, score = m - O_p at the start, and a one comes
// in at the bottom of the horizontal plus-delta in every step.
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
constexpr int kWarmup = 96;                    // bases a piece's walk starts in front of it: >= m + k2 (89 at most), a multiple of 4

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
    uint32_t o, k_o;  // the anchored walk (set_overhang): O_p and k'_p; o = 0: none
};

ADAPTERS_FN uint32_t edits_allowed(uint32_t m, uint32_t errors_percent) { return m * errors_percent / 100u; }
constexpr int kMaxOverhang = kMaxBases - kMinBases;  // O
// O_p: the pattern bases that may be missing in front of the read's edge
ADAPTERS_FN uint32_t overhang_of(uint32_t m, uint32_t overhang) { return overhang < m - (uint32_t)kMinBases ? overhang : m - (uint32_t)kMinBases; }

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

// one text base whose match mask against the pattern is eq; top = 1 << (m - 1): pv, mv and the score at row m, nothing else (the
// middle search only asks whether the score is within k2)
ADAPTERS_FN void column_advance(Column *s, uint64_t eq, uint64_t top) {
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
}

// text base j (1-based): the column's step and the minimum's bookkeeping of the ends rule
ADAPTERS_FN void column_step(Column *s, uint64_t eq, uint64_t top, int32_t j) {
    column_advance(s, eq, top);
    if (s->score <= s->dmin) {  // <=: the largest j wins a tie
        s->dmin = s->score;
        s->jbest = j;
    }
}

// The anchored walk: the first o pattern bases cost nothing (D[i][0] = max(0, i - o)), the text is taken from its first base
// (D[0][j] = j).  o <= kMaxOverhang < 64.
ADAPTERS_FN void column_start_anchored(Column *s, uint32_t m, uint32_t o) {
    s->pv = ~0ull << o;
    s->mv = 0;
    s->score = (int32_t)(m - o);
    s->dmin = 0x7fffffff;
    s->jbest = 0;
}

ADAPTERS_FN void column_step_anchored(Column *s, uint64_t eq, uint64_t top, int32_t j) {
    const uint64_t pv = s->pv, mv = s->mv;
    const uint64_t xv = eq | mv;
    const uint64_t xh = (((eq & pv) + pv) ^ pv) | eq;
    uint64_t ph = mv | ~(xh | pv);
    uint64_t mh = pv & xh;
    s->score += (ph & top) ? 1 : 0;
    s->score -= (mh & top) ? 1 : 0;
    ph = (ph << 1) | 1ull;  // (row 0 counts up: D[0][j] - D[0][j - 1] = 1)
    mh <<= 1;
    s->pv = mh | ~(xv | ph);
    s->mv = ph & xv;
    if (s->score <= s->dmin) {
        s->dmin = s->score;
        s->jbest = j;
    }
}

// the columns an anchored walk needs of a text of n bases
ADAPTERS_FN int32_t anchored_columns(int32_t n, uint32_t m, uint32_t k_o) { return n < (int32_t)(m + k_o) ? n : (int32_t)(m + k_o); }

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

// The marks of one (piece, pattern) walk come as runs: hit ends at consecutive j give overlapping marks.  A walk keeps the current run
// [lo, hi) and hands a finished one to `flush`; hit ends arrive with ascending j.
struct MarkRun {
    int32_t lo = -1, hi = -1;  // hi < 0: no run
};
template <class Flush>
ADAPTERS_FN void mark_hit(MarkRun *r, int32_t j, int32_t m, Flush &&flush) {
    const int32_t lo = j > m ? j - m : 0;
    if (r->hi >= 0 && lo <= r->hi) {
        r->hi = j;
        return;
    }
    if (r->hi >= 0) flush(r->lo, r->hi);
    r->lo = lo;
    r->hi = j;
}
template <class Flush>
ADAPTERS_FN void mark_end(MarkRun *r, Flush &&flush) {
    if (r->hi >= 0) flush(r->lo, r->hi);
    r->hi = -1;
}

// The mark bitmap: bit (offset + i) says base i of the read at `offset` of the plane lies in B; 32-bit words, bit b of word w is
// bit 32 w + b.  A plane of plane_bytes has mark_words(plane_bytes) words.
ADAPTERS_FN uint64_t mark_words(uint64_t plane_bytes) { return (plane_bytes + 31) / 32; }

// [s, e) of a read of L bases from its two keys; false: s >= e, nothing is left
ADAPTERS_FN bool kept_range(uint32_t key_head, uint32_t key_tail, int64_t L, int64_t *s, int64_t *e) {
    *s = (int64_t)(key_head >> 8);
    *e = L - (int64_t)(key_tail >> 8);
    return *s < *e;
}

// One 32-bit word of the child walk.  `free_bits`: the bases of this word that lie in [s, e) and outside B; `carry`: whether the base
// in front of the word was such a base.  A child starts at every bit of *starts and ends in front of every bit of *ends; the
// k-th start and the k-th end of a read belong to one child.  (A child that reaches e ends at the bit of e, which is never free.)
ADAPTERS_FN void child_edges(uint32_t free_bits, uint32_t carry, uint32_t *starts, uint32_t *ends) {
    const uint32_t before = (free_bits << 1) | (carry & 1u);
    *starts = free_bits & ~before;
    *ends = ~free_bits & before;
}

// What the child walk of a read comes to: n children found, whether an end hit or a mark inside [s, e) was seen
ADAPTERS_FN int64_t split_summary(bool end_hit, bool any_mark, int64_t n, int64_t L, int32_t first_start, int32_t last_end, int32_t *first,
                                  int32_t *last) {
    if (!end_hit && !any_mark) {
        *first = 0;
        *last = (int32_t)L;
        return 0;
    }
    *first = n ? first_start : -1;
    *last = n ? last_end : -1;
    return n;
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

// --adapter_overhang: O_p and k'_p of every pattern; false for O outside 0..kMaxOverhang
inline bool set_overhang(std::vector<Pattern> *patterns, int errors_percent, int overhang) {
    if (overhang < 0 || overhang > kMaxOverhang) return false;
    for (Pattern &p : *patterns) {
        p.o = overhang_of(p.m, (uint32_t)overhang);
        p.k_o = edits_allowed(p.m - p.o, (uint32_t)errors_percent);
    }
    return true;
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
        if (pat.o == 0u) continue;
        column_start_anchored(&col, pat.m, pat.o);
        const int64_t cols = anchored_columns((int32_t)n, pat.m, pat.k_o);
        for (int64_t j = 0; j < cols; ++j) {
            const uint8_t c = side ? read[L - 1 - j] : read[j];
            column_step_anchored(&col, select_eq(peq, code_of(c)), top, (int32_t)(j + 1));
        }
        if (n >= 1 && col.dmin <= (int32_t)pat.k_o) {
            const uint32_t mine = ((uint32_t)col.jbest << 8) | p;
            if (mine > key) key = mine;
        }
    }
    return key;
}

// The serial walk of --split_adapters for one read: the kernel's oracle.  Sets marked[i] = 1 for every base of B (marked has L
// entries, zero before).  Reads read[0, L) and nothing else.
inline void middle_marks(const uint8_t *read, int64_t L, const Pattern *patterns, uint32_t n_patterns, uint32_t split_errors_percent,
                         uint8_t *marked) {
    for (uint32_t p = 0; p < n_patterns; ++p) {
        const Pattern &pat = patterns[p];
        const int32_t k2 = (int32_t)edits_allowed(pat.m, split_errors_percent);
        const uint64_t top = 1ull << (pat.m - 1);
        Column col;
        column_start(&col, pat.m);
        MarkRun run;
        auto flush = [&](int32_t lo, int32_t hi) {
            for (int32_t i = lo; i < hi; ++i) marked[i] = 1;
        };
        for (int64_t j = 0; j < L; ++j) {
            column_advance(&col, select_eq(pat.peq_head, code_of(read[j])), top);
            if (col.score <= k2) mark_hit(&run, (int32_t)(j + 1), (int32_t)pat.m, flush);
        }
        mark_end(&run, flush);
    }
}

// The same marks piece by piece, pieces of S bases: every piece walks from max(0, a - kWarmup) and reports the hit ends in (a, b].
// What the kernel does, serially; equal to middle_marks by the argument at the top.
inline void middle_marks_pieces(const uint8_t *read, int64_t L, int64_t S, const Pattern *patterns, uint32_t n_patterns,
                                uint32_t split_errors_percent, uint8_t *marked) {
    for (int64_t a = 0; a < L; a += S) {
        const int64_t b = a + S < L ? a + S : L, from = a > kWarmup ? a - kWarmup : 0;
        for (uint32_t p = 0; p < n_patterns; ++p) {
            const Pattern &pat = patterns[p];
            const int32_t k2 = (int32_t)edits_allowed(pat.m, split_errors_percent);
            const uint64_t top = 1ull << (pat.m - 1);
            Column col;
            column_start(&col, pat.m);
            MarkRun run;
            auto flush = [&](int32_t lo, int32_t hi) {
                for (int32_t i = lo; i < hi; ++i) marked[i] = 1;
            };
            for (int64_t j = from; j < b; ++j) {
                column_advance(&col, select_eq(pat.peq_head, code_of(read[j])), top);
                if (j >= a && col.score <= k2) mark_hit(&run, (int32_t)(j + 1), (int32_t)pat.m, flush);
            }
            mark_end(&run, flush);
        }
    }
}

// The children of one read from its keys and its marks (marked[0, L)), by the word walk the kernel makes: ranges gets (start, end)
// pairs appended; returns their number and sets first / last.
inline int64_t split_children(uint32_t key_head, uint32_t key_tail, int64_t L, const uint8_t *marked, std::vector<int32_t> *ranges, int32_t *first,
                              int32_t *last) {
    int64_t s, e;
    const bool end_hit = (key_head | key_tail) != 0u;
    if (!kept_range(key_head, key_tail, L, &s, &e)) return split_summary(end_hit, false, 0, L, -1, -1, first, last);  // (no end hit: L = 0)
    std::vector<int32_t> st, en;
    bool any_mark = false;
    uint32_t carry = 0;
    for (int64_t w = s >> 5; w <= e >> 5; ++w) {  // (the word of e too: a child that reaches e ends there)
        uint32_t free_bits = 0;
        for (int b = 0; b < 32; ++b) {
            const int64_t i = 32 * w + b;
            if (i < s || i >= e) continue;
            if (marked[i]) any_mark = true;
            else free_bits |= 1u << b;
        }
        uint32_t starts, ends;
        child_edges(free_bits, carry, &starts, &ends);
        for (int b = 0; b < 32; ++b) {
            if ((starts >> b) & 1u) st.push_back((int32_t)(32 * w + b));
            if ((ends >> b) & 1u) en.push_back((int32_t)(32 * w + b));
        }
        carry = free_bits >> 31;
    }
    const int64_t n = split_summary(end_hit, any_mark, (int64_t)st.size(), L, st.empty() ? -1 : st.front(), en.empty() ? -1 : en.back(), first, last);
    for (int64_t k = 0; k < n; ++k) {
        ranges->push_back(st[(size_t)k]);
        ranges->push_back(en[(size_t)k]);
    }
    return n;
}

}  // namespace adapters
