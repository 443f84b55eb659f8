// fold_common.h — the parts of the k-mer window folds, shared by the one-lane kernel (score_kmer.hip: k_kmer_fold) and the wave
// kernels of the cooperative path (score_kmer_long.hip); the counterpart of cover_common.h for the second stage of k-mer mode.
//   kFoldModes      what each of k_kmer_fold's seven modes is: the only place where mode numbers mean something in device code
//   ZeroRunRule     which zero runs are bad ranges (src/read.cpp:89-130), and zero_run_word: the runs of one 32-bit word
//   FoldRow         the coverage row as one lane sees it: the LDS ring or the two global streams, whole reads and child slices
//   fold_word_*     the steady state of one word of 32 positions: floating point, the integer grid (fold_grid_tab.h), events
//   child_word_positions / fold_positions   the per-position forms: children inside their read's lane, the head and tail of a read
#pragma once

#include "score_kmer_common.h"

// ---- the modes of k_kmer_fold ----------------------------------------------------------------------------------------------------
// MODE 0: parent only (no --trim/--split).  MODE 1: parent + count children, bit by bit.  MODE 2: emit children.
// MODE 4: emit children with the zero-run events found at word level and a branch-light bit loop (same condition as 3).
// MODE 3: parent + count children at WORD level — a zero run can only be a bad range if it starts at position 0, reaches
// the end of the read, or is at least --split long; with --split >= 32 (or unset) every such run crosses a 32-bit word
// boundary, so the runs that lie inside one word never matter and the parent keeps MODE 0's branch-free steady state.
// MODE 5: the word-level events of MODE 3 once more, without any floating point: writes every child's (start, end) and its
// read's index at the child's place in the CSR.  MODE 6: ONE LANE PER CHILD, children in descending order of length — a child
// is a read of its own (src/read.cpp:131-137: Read(child name, seq + start, ...)), so its lane runs MODE 0's branch-free
// recurrence on the parent's coverage bits [start, end) (the row words funnel-shifted by start mod 32) and writes the child's
// mean / window / pass flag.  5 + 6 replace MODE 4, whose 32 predicated positions per word carry the event machinery through
// every bit (67 of the 98 ms per 10^11 positions of C4's folds).
enum FoldWindow { kWinNone, kWinWords, kWinBits, kWinChildWords };
enum FoldEvents { kEvNone, kEvWord, kEvBit };
enum FoldOut : unsigned {
    kOutRead = 1,          // the read's mean_q / window_q / passed
    kOutCount = 2,         // n_child of the read
    kOutInline = 4,        // the first kInlineChildren ranges of the read, beside it (FoldArgs::inline_ranges)
    kOutRanges = 8,        // every child's range at its place in the CSR (needs child_offsets)
    kOutParent = 16,       // ... and its read's index
    kOutChildScores = 32,  // ... and its mean / window / passed, from the child's recurrence carried in the read's lane
    kOutOwnScores = 64,    // the slot is a child: its own scores
};
struct FoldMode {
    bool child;         // the slot is a child — a slice [start, end) of its parent's row — not a read
    bool leaves_long;   // slots of at least FoldArgs::long_min bases are the cooperative path's: not live here
    FoldWindow window;  // the slot's own window: none; a word at a time (head shortcut, steady state), per position at its head and
                        // tail; every position on its own; or not the read's at all but its children's, 32 predicated positions per word
    FoldEvents events;  // zero runs -> bad ranges -> children: not looked for, per word, or per bit
    unsigned out;       // what the lane writes
};
constexpr FoldMode kFoldModes[7] = {
    /* 0 */ {false, true, kWinWords, kEvNone, kOutRead},
    /* 1 */ {false, false, kWinBits, kEvBit, kOutRead | kOutCount},
    /* 2 */ {false, false, kWinBits, kEvBit, kOutRanges | kOutChildScores},
    /* 3 */ {false, true, kWinWords, kEvWord, kOutRead | kOutCount | kOutInline},
    /* 4 */ {false, false, kWinChildWords, kEvWord, kOutRanges | kOutChildScores},
    /* 5 */ {false, true, kWinNone, kEvWord, kOutRanges | kOutParent},
    /* 6 */ {true, true, kWinWords, kEvNone, kOutOwnScores},
};

// ---- zero runs -> bad ranges (src/read.cpp:89-130) -------------------------------------------------------------------------------
struct ZeroRunRule {
    bool split_set, trim;
    int split;
    __device__ __forceinline__ explicit ZeroRunRule(const flx_params &p) : split_set(p.split_set != 0), trim(p.trim != 0), split(p.split) {}
    // the run [zs, end) that a covered base ended: bad if --split long, or, under --trim, at the start of the read
    __device__ __forceinline__ bool bad_run(int zs, int end) const { return (split_set && end - zs >= split) || (trim && zs == 0); }
    // the run [zs, end) the read ends inside: under --trim bad unless it is the whole read
    __device__ __forceinline__ bool bad_run_at_end(int zs, int end) const { return (split_set && end - zs >= split) || (trim && zs > 0); }
};

// The children found in a read's lane: the current candidate and, for the modes that score children there, its recurrence.
struct Children {
    Win C = {0, 0.0, 0.0};
    Win S = {0, 0.0, 0.0};  // snapshot of C at the start of the current zero run
    int cs = 0;             // start of the current child candidate
    int zs = -1;            // start of the current zero run (-1: none)
    bool any_bad = false;
    uint32_t n = 0;
};

// The zero runs of one word, at word level: only the run that REACHED this word can be bad (one inside the word is shorter than 32),
// and it ends at the word's first covered base; the word may end inside a new run.
struct ZeroRunWord {
    int ev_end;  // bit of the word at which a bad range ended (-1: none) — the child [cs, ev_zs) is complete, a new one starts there
    int ev_zs;
    int snap;    // bit of the word at which a new zero run starts (-1: none): the child's state there is what a bad range would keep
};
__device__ __forceinline__ ZeroRunWord zero_run_word(const ZeroRunRule &rule, uint32_t lead_w, int j0, int L, int &zs) {
    ZeroRunWord r = {-1, 0, -1};
    if (j0 >= L) return r;  // behind the read's end (the wave's longest read is not over)
    const int v = min(32, L - j0);  // valid bits of this word
    const uint32_t w = v < 32 ? (lead_w & ((1u << v) - 1u)) : lead_w;
    if (j0 == 0 && !(w & 1u)) zs = 0;  // the read starts inside a zero run
    if (w != 0) {
        if (zs >= 0) {  // the run [zs, j) that reached this word ends at its first covered base
            const int f = __ffs(w) - 1;
            if (rule.bad_run(zs, j0 + f)) {
                r.ev_end = f;
                r.ev_zs = zs;
            }
            zs = -1;
        }
        const int top = 32 - __clz(w);  // one past the last covered base of the word
        if (top < v) {                  // the word ends inside a new zero run
            zs = j0 + top;
            r.snap = top;
        }
    } else if (zs < 0) {
        zs = j0;
        r.snap = 0;
    }
    return r;
}

template <unsigned OUT>
__device__ __forceinline__ void emit_child(const FoldArgs &a, uint32_t rid, uint64_t cbase, uint32_t &nchild, int start, int end, const Win &st) {
    if (end <= start) return;
    const uint64_t at = cbase + nchild;
    if (OUT & kOutRanges) {
        a.child_ranges[2 * at] = start;
        a.child_ranges[2 * at + 1] = end;
    }
    if (OUT & kOutParent) a.child_parent[at] = rid;
    if ((OUT & kOutInline) && a.inline_ranges && nchild < (uint32_t)kInlineChildren) {
        int32_t *slot = a.inline_ranges + ((size_t)rid * kInlineChildren + nchild) * 2;
        slot[0] = start;
        slot[1] = end;
    }
    if (OUT & kOutChildScores) {
        const int len = end - start;
        const double mean = 100.0 * (double)st.cnt / (double)len;
        const double window = window_result(a, len, st.cnt, st.mn);
        a.child_mean_q[at] = mean;
        a.child_window_q[at] = window;
        a.child_passed[at] = cutoffs(a.p, len, mean, window);
    }
    ++nchild;
}

// ---- the row as seen by one lane -------------------------------------------------------------------------------------------------
// Two word streams over the read's coverage row — the leading edge (position j) and the trailing edge (position
// j - ws).  Each lane walks its own row: 64 lanes = 64 distinct lines per load instruction, and the rows of all resident
// lanes do not fit L1 / L2 together, so a line is gone again before the lane comes back to it — every load of a new piece
// is a far request (55 G/s, profiles/r03_microbench.txt).
//   RING (default): the row is read ONCE, 64 bytes per lane at a time (four 16-byte loads issued back to back to one
//   half line, a block ahead of their use), and parked in a per-lane ring of words in LDS (word k of lane l at
//   ((k mod R) * 64 + l): every access of a wave is conflict free and touches only the lane's own words, so no barrier).
//   Both edges then come out of the ring with ds_read_b32: one far request per 512 positions instead of two per 128,
//   which had made the folds request bound (round 2: 28 of the 36 ms per 10^11 positions).
//   !RING: both streams straight from global memory in 16-byte blocks (windows too long for the ring).
// CHILD: bit p of the child is bit p + bit_off of the row, so 32 child positions from position p on are row words
// (p + bit_off) / 32 and the next one, funnel-shifted by (p + bit_off) mod 32.
struct WStream { uint4 cur, nxt; int blk; };
struct FoldRow {
    const uint32_t *row;
    int n_words;       // words of the row that exist behind `row`
    uint32_t bit_off;  // CHILD: the child starts at bit `bit_off` (0..127) of row[0]
    uint32_t *ring;    // RING: this lane's word 0 of the ring
    int R;             // ... of R words, a power of two >= 16 + ceil(ws / 32) + 2
    uint4 nq[4];       // the block after the newest one in the ring
    int have_blk;      // newest block in the ring (wave-uniform: every lane is at the same position)
    WStream lead, trail;

    __device__ __forceinline__ uint4 ldq(int b) const {
        return (b * 4 < n_words) ? *reinterpret_cast<const uint4 *>(row + 4 * (size_t)b) : make_uint4(0u, 0u, 0u, 0u);
    }
    template <bool RING>
    __device__ __forceinline__ void begin() {
        lead = {make_uint4(0u, 0u, 0u, 0u), make_uint4(0u, 0u, 0u, 0u), 0};
        if (!RING) lead = {ldq(0), ldq(1), 0};
        trail = lead;
        have_blk = -1;
        if (RING) {
#pragma unroll
            for (int q = 0; q < 4; ++q) nq[q] = ldq(q);
        }
    }
    __device__ __forceinline__ void advance(WStream &st, int b) const {  // streams only move forward, one block at a time
        if (b != st.blk) {
            st.cur = st.nxt;
            st.blk = b;
            st.nxt = ldq(b + 1);
        }
    }
    __device__ __forceinline__ uint32_t word(const WStream &st, int wi) const {  // wi inside block st.blk or st.blk + 1
        // (selects, no reference to one of the two blocks: a reference makes the compiler keep the stream in scratch memory)
        const bool cur = (wi >> 2) == st.blk;
        const int c = wi & 3;
        const uint4 c4 = st.cur, n4 = st.nxt;
        const uint32_t x = cur ? c4.x : n4.x, y = cur ? c4.y : n4.y, z = cur ? c4.z : n4.z, w = cur ? c4.w : n4.w;
        const uint32_t v = c == 0 ? x : c == 1 ? y : c == 2 ? z : w;
        return wi < n_words ? v : 0u;  // the padding of the last block is not coverage
    }
    __device__ __forceinline__ void ring_fill(int wi) {  // word wi (and everything up to the end of its block) into the ring; wi only moves forward
        const int b = wi >> 4;
        if (b > have_blk) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int k = (b * 16 + 4 * q) & (R - 1);
                ring[(k + 0) * 64] = nq[q].x; ring[(k + 1) * 64] = nq[q].y; ring[(k + 2) * 64] = nq[q].z; ring[(k + 3) * 64] = nq[q].w;
            }
            have_blk = b;
#pragma unroll
            for (int q = 0; q < 4; ++q) nq[q] = ldq((b + 1) * 4 + q);
        }
    }
    __device__ __forceinline__ uint32_t ring_word(int wi) const { return wi < n_words ? ring[(wi & (R - 1)) * 64] : 0u; }
    template <bool RING>
    __device__ __forceinline__ uint32_t trail_bits(int p) {  // CHILD; any p >= 0 behind the leading edge, moving forward
        const int t = p + (int)bit_off, w = t >> 5;
        uint32_t lo, hi;
        if (RING) { lo = ring_word(w); hi = ring_word(w + 1); }
        else { advance(trail, w >> 2); lo = word(trail, w); hi = word(trail, w + 1); }
        return __builtin_amdgcn_alignbit(hi, lo, (unsigned)(t & 31));
    }
    template <bool RING, bool CHILD>
    __device__ __forceinline__ uint32_t lead_word(int wi) {  // the word holding the leading edge
        if (CHILD) {  // (wi moving forward) row words wi + bit_off / 32 and the next one
            const int w = wi + (int)(bit_off >> 5);
            uint32_t lo, hi;
            if (RING) { ring_fill(w + 1); lo = ring_word(w); hi = ring_word(w + 1); }
            else { advance(lead, w >> 2); lo = word(lead, w); hi = word(lead, w + 1); }
            return __builtin_amdgcn_alignbit(hi, lo, bit_off & 31u);
        }
        if (RING) { ring_fill(wi); return ring_word(wi); }
        advance(lead, wi >> 2);
        return word(lead, wi);
    }
    template <bool RING, bool CHILD>
    __device__ __forceinline__ uint32_t trail_word(int wi) {  // words of the trailing edge: never ahead of the leading one
        if (CHILD) return trail_bits<RING>(wi << 5);
        if (RING) return ring_word(wi);
        advance(trail, wi >> 2);
        return word(trail, wi);
    }
    template <bool RING, bool CHILD>
    __device__ __forceinline__ uint32_t trail32(int p) {  // positions p .. p + 31 (p >= 0) of the trailing edge
        if (CHILD) return trail_bits<RING>(p);
        const int sh = p & 31, twi = p >> 5;
        const uint32_t t0 = trail_word<RING, CHILD>(twi);
        return sh ? __builtin_amdgcn_alignbit(trail_word<RING, CHILD>(twi + 1), t0, (unsigned)sh) : t0;
    }
};

// ---- the steady state of one word: 32 positions, every lane active, no per-bit control flow --------------------------------------
// In floating point.  w - q[j-ws]/ws and + q[j]/ws with q in {0.0, 1.0} (src/read.cpp:228-229) as fma(bit, -+delta, w): the product
// is exact (0 or delta), so the one rounding of the fma is the rounding of the reference's subtraction / addition, and adding a zero
// product leaves w as it is.  7 VALU instructions per position; the form with masked deltas and a plain subtraction / addition took 9
// and lost — the folds are VALU bound.  ROUNDS: four rounds of eight steps, not 32 unrolled, for the callers that replay a word in
// the middle of other state (the integer grid, the wave kernel): unrolled there, the compiler converts all 64 bits to doubles ahead
// of the chain and the kernel needs 122 registers, or spills.
template <bool ROUNDS>
__device__ __forceinline__ void fold_word_fp(double &w, double &mn, uint32_t lead_w, uint32_t tw, double delta) {
    constexpr int kRound = ROUNDS ? 8 : 32;
#pragma unroll 1
    for (int i0 = 0; i0 < 32; i0 += kRound) {
#pragma unroll
        for (int i = 0; i < kRound; ++i) {
            const double lb = (double)__builtin_amdgcn_ubfe(lead_w, i0 + i, 1);
            const double tb = (double)__builtin_amdgcn_ubfe(tw, i0 + i, 1);
            w = fma(tb, -delta, w);
            w = fma(lb, delta, w);
            mn = fmin(mn, w);
        }
    }
}

// On the integer grid (fold_grid_tab.h).  In LDS, in front of the rings: the table of the +-1 walk of four positions, indexed by
// (new nibble << 4 | old nibble): two dwords, {lowest prefix, -(highest prefix)} and {total, -total} as pairs of 16-bit integers
// (packed adds and minima carry both at once) — one copy: 8 and 16 copies, a lane reading copy lane % copies so that lanes with
// different nibble pairs rarely meet in one bank, measured no different; the gathers are not what bounds the kernel — and behind it
// the grid table itself (GridTab: d* and the lower bound per binade, 8 dwords per entry): a regime begins in the middle of the
// steady state, and a load from the kernel's arguments there costs the whole wave a trip to memory.
constexpr int kGridTabAt = 512;                     // dword index of the grid table
constexpr int kGridLdsWords = kGridTabAt + 8 * 32;  // dwords in front of the rings
__device__ __forceinline__ void grid_lds_fill(uint32_t *lds, const GridTab &gt) {  // by the whole workgroup, with its barrier
    for (int i = threadIdx.x; i < GridTab::kMax; i += blockDim.x) {
        lds[kGridTabAt + 8 * i + 0] = (uint32_t)__double2loint(gt.dstar[i]);
        lds[kGridTabAt + 8 * i + 1] = (uint32_t)__double2hiint(gt.dstar[i]);
        lds[kGridTabAt + 8 * i + 2] = (uint32_t)__double2loint(gt.lv[i]);
        lds[kGridTabAt + 8 * i + 3] = (uint32_t)__double2hiint(gt.lv[i]);
        lds[kGridTabAt + 8 * i + 4] = (uint32_t)gt.top[i];
    }
    for (int idx = threadIdx.x; idx < 256; idx += blockDim.x) {
        int t = 0, mp = 0, xp = 0;
        for (int i = 0; i < 4; ++i) {
            t += ((idx >> (4 + i)) & 1) - ((idx >> i) & 1);
            mp = min(mp, t);
            xp = max(xp, t);
        }
        lds[2 * idx] = ((uint32_t)mp & 0xffffu) | ((uint32_t)(-xp) << 16);
        lds[2 * idx + 1] = ((uint32_t)t & 0xffffu) | ((uint32_t)(-t) << 16);
    }
    __syncthreads();
}
// The regime of one lane's window: w = r.wb + c * r.ds while it holds; lowest c so far in cmin.
struct GridLane {
    GridRegime r = {0.0, 0.0, 0x7fffffff, (int)0x80000000};
    int c = 0, cmin = 0;
    bool on = false;  // wave-uniform: the steady state has begun (and not ended: it is one stretch of words, it does not begin again)
};
__device__ __forceinline__ void grid_flush(const GridLane &g, Win &P) {  // the regime's state as the recurrence's
    P.mn = fmin(P.mn, grid_value(g.r, g.cmin));
    P.w = grid_value(g.r, g.c);
}
__device__ __forceinline__ void grid_begin(GridLane &g, double w, const uint32_t *lds, const FoldArgs &a) {  // a regime from w on
    double ds = 0.0, lv = 0.0;
    int top = 0;
    const int idx = grid_binade(w) - a.gt.e0;
    if (w > 0.0 && idx >= 0 && idx < a.gt.n) {
        const uint32_t *e = lds + kGridTabAt + 8 * idx;
        ds = __hiloint2double((int)e[1], (int)e[0]);
        if (ds > 0.0) {  // (a tie: the rest of the entry is not read)
            lv = __hiloint2double((int)e[3], (int)e[2]);
            top = (int)e[4];
        }
    }
    g.r = grid_regime_begin(w, ds, lv, top, a.ws_d);
    g.c = g.cmin = 0;
}
__device__ __forceinline__ void fold_word_grid(GridLane &g, Win &P, uint32_t lead_w, uint32_t tw, const uint32_t *lds, const FoldArgs &a) {
    if (!g.on) {
        grid_begin(g, P.w, lds, a);
        g.on = true;
    }
    typedef short s16x2 __attribute__((ext_vector_type(2)));
    // the (new, old) nibble pairs of the word: byte k of `even` = nibbles 2k, of `odd` = nibbles 2k + 1
    const uint32_t odd = (lead_w & 0xF0F0F0F0u) | ((tw >> 4) & 0x0F0F0F0Fu);
    const uint32_t even = ((lead_w << 4) & 0xF0F0F0F0u) | (tw & 0x0F0F0F0Fu);
    const uint2 *walk = reinterpret_cast<const uint2 *>(lds);
    s16x2 run = {0, 0}, ext = {0, 0};  // {prefix, -prefix} so far; {lowest prefix, -(highest prefix)}
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const uint32_t idx = ((k & 1 ? odd : even) >> (8 * (k >> 1))) & 0xffu;
        const uint2 e = walk[idx];
        ext = __builtin_elementwise_min(ext, run + __builtin_bit_cast(s16x2, e.x));
        run = run + __builtin_bit_cast(s16x2, e.y);
    }
    const int mp = ext.x, xp = -(int)ext.y, t = run.x;
    // not a no-op (a word of zeros on both edges changes nothing in any regime) and outside the regime: this lane's word in FP
    const bool slow = (lead_w | tw) != 0u && !(g.c + mp >= g.r.lo && g.c + xp <= g.r.hi);
    if (!__any(slow)) {
        g.cmin = min(g.cmin, g.c + mp);
        g.c += t;
        return;
    }
    if (!slow) {
        g.cmin = min(g.cmin, g.c + mp);
        g.c += t;
        lead_w = tw = 0;  // (32 exact no-ops below)
    } else {
        grid_flush(g, P);
    }
    fold_word_fp<true>(P.w, P.mn, lead_w, tw, a.delta);
    if (slow) grid_begin(g, P.w, lds, a);
}

// By events (FLX_KMER_FOLD_EVENTS=1; measured: not faster).  Round-3 review, item 5: only the positions where the two edges DIFFER
// change w for certain (one exact step each); where both are 0 nothing happens, and where both are 1 the step is fl(fl(w - d) + d),
// which is w itself unless the subtraction leaves w's binade — checked once per stretch of such positions, with fold_word_fp as the
// fallback for a word where it fails.  Lanes diverge (a wave runs as many rounds as its busiest lane has events).
// Returns true when no lane of the wave needs the fallback; else the lanes that are done have their word zeroed (32 exact no-ops).
__device__ __forceinline__ bool fold_word_events(Win &P, uint32_t &lead_w, uint32_t &tw, double delta) {
    const double w0 = P.w, mn0 = P.mn;
    const uint32_t both = lead_w & tw;
    uint32_t ev = lead_w ^ tw, handled = 0;
    bool slow = false;
    for (;;) {
        const int i = ev ? __ffs(ev) - 1 : 32;
        const uint32_t upto = i == 32 ? 0xffffffffu : ((1u << i) - 1u);
        if (both & upto & ~handled) {
            double t = P.w - delta;
            t = t + delta;
            if (t != P.w) { slow = true; break; }
        }
        if (i == 32) break;
        if ((lead_w >> i) & 1u) {
            P.w = P.w + delta;
        } else {
            P.w = P.w - delta;
            P.mn = fmin(P.mn, P.w);
        }
        handled = upto | (1u << i);
        ev &= ev - 1;
    }
    if (!__any(slow)) return true;
    if (!slow) {
        lead_w = tw = 0;
    } else {
        P.w = w0;
        P.mn = mn0;
    }
    return false;
}

// ---- per position ----------------------------------------------------------------------------------------------------------------
// The children of a read inside its lane, a word at a time: the events of the word (zero_run_word), then 32 predicated positions of
// the current child's recurrence.
template <bool RING, unsigned OUT>
__device__ __forceinline__ void child_word_positions(const FoldArgs &a, FoldRow &row, int j0, int L, uint32_t lead_w, const ZeroRunWord &z, Children &K,
                                                     uint32_t rid, uint64_t cbase) {
    const int ws = a.ws;
    const unsigned int d_lo = (unsigned int)(__double_as_longlong(a.delta) & 0xffffffffll);
    const unsigned int d_hi = (unsigned int)(__double_as_longlong(a.delta) >> 32);
    // trailing window of the 32 positions (positions before the read count as uncovered; they are never used,
    // a child's trailing edge lies inside the child)
    const int tj0 = j0 - ws;
    uint32_t tw = 0;
    if (tj0 > -32) {
        const int twi = tj0 >> 5, sh = tj0 & 31;  // twi == -1 for the word that straddles position 0
        const uint32_t lo = twi >= 0 ? row.trail_word<RING, false>(twi) : 0u;
        tw = sh ? __builtin_amdgcn_alignbit(row.trail_word<RING, false>(twi + 1), lo, (unsigned)sh) : lo;
    }
    Win &C = K.C, &S = K.S;
#pragma unroll
    for (int i = 0; i < 32; ++i) {
        const int j = j0 + i;
        if (i == z.ev_end) {  // a bad range ended here: the child [cs, ev_zs) is complete, a new one starts at j
            K.any_bad = true;
            emit_child<OUT>(a, rid, cbase, K.n, K.cs, z.ev_zs, S);
            K.cs = j;
            C.cnt = 0;
            C.w = 0.0;
            C.mn = 0.0;
        }
        if (i == z.snap) {  // state of the current child at the start of a zero run that may turn out bad
            S.cnt = C.cnt;
            S.mn = C.mn;
        }
        const bool act = j < L;
        const int k = j - K.cs;
        const int ml = __builtin_amdgcn_sbfe((int)lead_w, i, 1);  // 0 or -1 (bits beyond L are 0)
        const int mt = __builtin_amdgcn_sbfe((int)tw, i, 1);
        C.cnt -= ml;
        if (act && k == ws - 1) {
            C.w = (double)C.cnt / a.ws_d;
            C.mn = C.w;
        }
        const bool steady = act && k >= ws;
        const int ms = steady ? -1 : 0;
        const double dl = __hiloint2double((int)(d_hi & (unsigned)(ml & ms)), (int)(d_lo & (unsigned)(ml & ms)));
        const double dt = __hiloint2double((int)(d_hi & (unsigned)(mt & ms)), (int)(d_lo & (unsigned)(mt & ms)));
        C.w -= dt;  // exact no-ops outside the steady state
        C.w += dl;
        const double m2 = fmin(C.mn, C.w);
        C.mn = steady ? m2 : C.mn;
    }
}

// The head and the tail of a read — and, with per-bit events, all of it: one position at a time, lanes behind their read's end idle.
template <bool RING, bool CHILD, FoldEvents EVENTS, unsigned OUT>
__device__ __forceinline__ void fold_positions(const FoldArgs &a, FoldRow &row, int j0, int L, int Lmax, uint32_t lead_w, uint32_t &trail_w, Win &P,
                                               const ZeroRunRule &rule, Children &K, uint32_t rid, uint64_t cbase) {
    const int ws = a.ws;
    const double delta = a.delta;
    for (int jj = 0; jj < 32; ++jj) {
        const int j = j0 + jj;
        if (j >= Lmax) break;
        const int tj = j - ws;
        if (tj >= 0 && ((tj & 31) == 0 || jj == 0)) {
            trail_w = row.trail_word<RING, CHILD>(tj >> 5);
        }
        const bool act = j < L;
        const uint32_t b = act ? ((lead_w >> (j & 31)) & 1u) : 0u;
        const uint32_t tb = (act && tj >= 0) ? ((trail_w >> (tj & 31)) & 1u) : 0u;
        const double dl = b ? delta : 0.0;
        const double dt = tb ? delta : 0.0;

        if (act) {
            // ---- parent window (src/read.cpp:216-236) ----
            P.cnt += (int)b;
            if (j == ws - 1) {
                P.w = (double)P.cnt / a.ws_d;
                P.mn = P.w;
            } else if (j >= ws) {
                P.w -= dt;
                P.w += dl;
                if (P.w < P.mn) P.mn = P.w;
            }
            if (EVENTS == kEvBit) {
                // ---- zero runs -> bad ranges -> children (src/read.cpp:89-141) ----
                Win &C = K.C;
                if (b == 0 && K.zs < 0) {
                    K.zs = j;
                    K.S = C;
                }
                if (b == 1 && K.zs >= 0) {  // the run [zs, j) has ended
                    if (rule.bad_run(K.zs, j)) {
                        K.any_bad = true;
                        emit_child<OUT>(a, rid, cbase, K.n, K.cs, K.zs, K.S);
                        K.cs = j;
                        C.cnt = 0;
                        C.w = 0.0;
                        C.mn = 0.0;
                    }
                    K.zs = -1;
                }
                const int k = j - K.cs;  // position inside the current child
                C.cnt += (int)b;
                if (k == ws - 1) {
                    C.w = (double)C.cnt / a.ws_d;
                    C.mn = C.w;
                } else if (k >= ws) {
                    C.w -= dt;
                    C.w += dl;
                    if (C.w < C.mn) C.mn = C.w;
                }
            }
        }
    }
}
