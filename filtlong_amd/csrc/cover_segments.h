// cover_segments.h — how the coverage stage of k-mer mode cuts a long read into segments (host and device; the one copy that the
// cover kernels, the host side in cover_long.hip and the simulation tools/sim_cover_segments.cpp use).
//
// Coverage is a pure function of the read and the set: base i is covered iff a member 16-mer starts at some j in [i - 15, i]
// (src/read.cpp:43-58).  So a read can be cut anywhere, provided both sides see 15 bases of context.  Segment k of a read of L bases
// owns the bases [k * seg_bases, min(L, (k + 1) * seg_bases)) and is covered as a VIRTUAL READ [S, T) of its own, with 32 bases of
// context on either side where the read has them; of what that gives, only the owned bases — the emit range, in the virtual read's
// coordinates — are written and counted.  seg_bases is a multiple of 32, and so is S: the virtual read's plane pointer keeps its 16-byte
// alignment, its coverage row starts on a whole 32-bit word, and the words of an emit range are whole words no other segment writes.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FLX_SEG_HD __host__ __device__
#else
#define FLX_SEG_HD
#endif

constexpr int kCoverSegContext = 32;  // bases of context on either side of a segment (>= 15, a multiple of 32)

struct CoverSeg {
    int S, T;              // the virtual read: bases [S, T) of the read
    int emit_lo, emit_hi;  // the owned bases in the virtual read's coordinates: [emit_lo, emit_hi)
};

// segments of a read of L bases (seg_bases > 0, a multiple of 32)
FLX_SEG_HD inline long long flx_cover_seg_count(int L, int seg_bases) { return ((long long)L + seg_bases - 1) / seg_bases; }

FLX_SEG_HD inline CoverSeg flx_cover_seg(int L, int seg_bases, long long k) {
    const long long begin = k * seg_bases;
    const long long end = begin + seg_bases < (long long)L ? begin + seg_bases : (long long)L;
    const long long S = begin >= kCoverSegContext ? begin - kCoverSegContext : 0;
    const long long T = end + kCoverSegContext < (long long)L ? end + kCoverSegContext : (long long)L;
    CoverSeg s;
    s.S = (int)S;
    s.T = (int)T;
    s.emit_lo = (int)(begin - S);
    s.emit_hi = (int)(end - S);
    return s;
}

// A read's covered count / first covered base / last one (as the cover kernels give them: -1 / -1 for a read without coverage) out
// of its segments', which are in the virtual reads' coordinates: start from {0, -1, -1} and add the segments in any order.
struct CoverTotals {
    int count, first, last;
};
FLX_SEG_HD inline void flx_cover_seg_add(CoverTotals &t, int S, int count, int first, int last) {
    if (count <= 0) return;
    t.count += count;
    t.first = (t.first < 0 || S + first < t.first) ? S + first : t.first;
    t.last = S + last > t.last ? S + last : t.last;
}
