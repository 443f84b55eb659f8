// endtrim.h — --trim_ends_q: the low-quality ends of a read cut off, each end at the maximum of a running sum over the whole read (the
// rule of cutadapt -q and BWA -q without their early stop).  The record core of endtrim.hip, shared by the kernels and the host walk,
// and like qsplit.h / complexity.h plain C++ that a HIP kernel and a host program both include.  The reference has no counterpart.
//
// Everything is defined on integers, so any parallel decomposition gives the answer of the serial walk below.
//   error table   E[b] of qsplit.h (qsplit::kErrorTable): the error probability of quality byte b in units of 2^-32
//   threshold     t, 0 <= t < 2^32; for --trim_ends_q Q the t of qsplit::threshold(Q) = floor((100 - Q) / 100 * 2^32)
//   weight        w(b) = (int64)E[b] - (int64)t: positive for a base worse than the threshold, zero for one exactly on it
//   head cut      P(j) = sum of w(q[i]) for i < j, 0 <= j <= L, P(0) = 0; h = the SMALLEST j at which P takes its maximum (h = 0 when
//                 no P(j) > 0: ties keep more of the read)
//   tail cut      S(c) = sum of w(q[L - 1 - i]) for i < c; c = the smallest c at which S takes its maximum
//   both cuts     over the WHOLE read and independent of each other; the child rule is that of the adapter ends (adapters::child_of)
//                 with s = h and e = L - c: both 0: the read goes on as itself; s < e: one child [s, e); otherwise none and the read fails
//   bound         |w| < 2^32 and L < 2^31, so every sum stays below 2^63 in magnitude: the arithmetic is int64 throughout
//
// The associative form.  A PIECE is a run [a, b) of the read's bases, described in the read's own coordinates:
//   sum           the sum of w over the piece
//   pre, pre_at   the best prefix: max over a <= j <= b of the sum of w over [a, j), and the smallest j that reaches it (pre >= 0: j = a)
//   suf, suf_at   the best suffix: max over a <= e <= b of the sum of w over [e, b), and the LARGEST e that reaches it — the smallest
//                 length b - e (suf >= 0: e = b)
// Two adjacent pieces A = [a, m) and B = [m, b) combine to [a, b): the prefixes that end in B are worth A.sum + B.pre, the suffixes
// that begin in A are worth A.suf + B.sum, and the piece further from the end in question is taken only when its value is STRICTLY
// greater — that is the tie rule (the prefix of B that ends at m is worth A.sum <= A.pre, so A keeps a tie; likewise for the suffix).
// The rule is associative, so spans, waves, chunks and ranks all give the serial walk's answer.  The whole read's piece has
// h = pre_at and c = L - suf_at.
#pragma once

#include <stdint.h>

#include "qsplit.h"

#if defined(__HIPCC__)
#define ENDTRIM_FN __host__ __device__ __forceinline__
#else
#define ENDTRIM_FN inline
#endif

namespace endtrim {

constexpr int kSpan = 16384;  // quality bytes per work item of the kernel (flx_endtrim_span): 16 steps of a wave's 64 x 16 bytes

struct Piece {
    int64_t sum, pre, suf;
    uint32_t pre_at, suf_at;
};

ENDTRIM_FN int64_t weight(uint32_t e, uint64_t t) { return (int64_t)e - (int64_t)t; }

// the piece without a base, in front of base `at`
ENDTRIM_FN Piece empty_at(uint32_t at) { return Piece{0, 0, 0, at, at}; }

// a and b adjacent, a in front
ENDTRIM_FN Piece combine(const Piece &a, const Piece &b) {
    Piece r;
    r.sum = a.sum + b.sum;
    const int64_t pb = a.sum + b.pre, sa = a.suf + b.sum;
    const bool later_prefix = pb > a.pre, earlier_suffix = sa > b.suf;
    r.pre = later_prefix ? pb : a.pre;
    r.pre_at = later_prefix ? b.pre_at : a.pre_at;
    r.suf = earlier_suffix ? sa : b.suf;
    r.suf_at = earlier_suffix ? a.suf_at : b.suf_at;
    return r;
}

// the piece [a, b) by a walk over its bases: what a lane does with its 16 bytes, and the host with any piece
ENDTRIM_FN Piece piece_of(const uint8_t *qual, const uint32_t *table, uint32_t a, uint32_t b, uint64_t t) {
    Piece p = empty_at(a);
    // prefix sums P relative to a: the best prefix is the maximum of P with the smallest j, the best suffix is sum - the minimum of
    // P with the LARGEST j
    int64_t run = 0, lo = 0;
    uint32_t lo_at = a;
    for (uint32_t j = a; j < b; ++j) {
        run += weight(table[qual[j]], t);
        if (run > p.pre) {
            p.pre = run;
            p.pre_at = j + 1u;
        }
        if (run <= lo) {
            lo = run;
            lo_at = j + 1u;
        }
    }
    p.sum = run;
    p.suf = run - lo;
    p.suf_at = lo_at;
    return p;
}

// The serial walk over one quality string: the kernels' oracle.  Reads qual[0, L) and nothing else; L <= 0 gives 0, 0.
inline void cuts_host(const uint8_t *qual, int64_t L, uint64_t t, uint32_t *h, uint32_t *c) {
    *h = 0;
    *c = 0;
    if (L <= 0) return;
    int64_t run = 0, best = 0;
    for (int64_t j = 0; j < L; ++j) {
        run += weight(qsplit::kErrorTable[qual[j]], t);
        if (run > best) {
            best = run;
            *h = (uint32_t)(j + 1);
        }
    }
    run = 0;
    best = 0;
    for (int64_t k = 0; k < L; ++k) {
        run += weight(qsplit::kErrorTable[qual[L - 1 - k]], t);
        if (run > best) {
            best = run;
            *c = (uint32_t)(k + 1);
        }
    }
}

// the same by pieces of `piece` bases combined in order (tests/endtrim_host.cpp: every decomposition against the walk above)
inline void cuts_by_pieces(const uint8_t *qual, int64_t L, uint64_t t, int64_t piece, uint32_t *h, uint32_t *c) {
    *h = 0;
    *c = 0;
    if (L <= 0 || piece <= 0) return;
    Piece all = empty_at(0);
    for (int64_t a = 0; a < L; a += piece) {
        const int64_t b = a + piece < L ? a + piece : L;
        all = combine(all, piece_of(qual, qsplit::kErrorTable, (uint32_t)a, (uint32_t)b, t));
    }
    *h = all.pre_at;
    *c = (uint32_t)L - all.suf_at;
}

// the child rule (adapters::child_of with the cuts in the place of the keys' cut lengths): the number of children, first and last
ENDTRIM_FN int child_of(uint32_t h, uint32_t c, int64_t L, int32_t *first, int32_t *last) {
    if ((h | c) == 0u) {
        *first = 0;
        *last = (int32_t)L;
        return 0;
    }
    const int64_t s = (int64_t)h, e = L - (int64_t)c;
    if (s < e) {
        *first = (int32_t)s;
        *last = (int32_t)e;
        return 1;
    }
    *first = -1;
    *last = -1;
    return 0;
}

}  // namespace endtrim
