// cover_common.h — what the coverage stage of k-mer mode shares: the stage's host entry (flx_kmer_cover_stage, defined in
// cover_wave.hip), the argument block of the wave-level kernels, and the ONE copy of every rule of the filter that more than one
// of them applies — the text verdict, text addressing and the seed probe, the exact pair probe and its search step, a piece's
// coverage word and a read's counts.  Kernels: cover_wave.hip (k_kmer_cover, the workgroup-per-read form "v2", and k_kmer_cover_w,
// the wave-level form of rounds 3-5), cover_queue.hip (k_kmer_cover_q, round 6, with lane_diagonals), cover_long.hip (the segment
// table and the reduce of the cooperative path).  Every function below is __forceinline__ and takes what it updates by reference:
// the kernels sit at the 64-register edge of 8 waves per SIMD, and against the copies these functions replaced no instantiation
// gained scratch, a spilled vector register or a memory instruction (profiles/cover_shared_core.md) — check that table again after
// changing a signature here.
// Reference semantics: src/read.cpp:43-58 (rolling 2-bit 16-mer, one set lookup per position, bases i-15..i marked on a hit).
#pragma once
#include "flx_internal.h"
#include "kmerset.h"
#include "cover_segments.h"

#ifndef FLX_COVER_THREADS
#define FLX_COVER_THREADS 256  // threads per workgroup of the wave-level cover kernels (their waves are independent)
#endif
#ifndef FLX_LOCUS_SEEDS
#define FLX_LOCUS_SEEDS 4  // seed attempts per span of the locus path
#endif
#ifndef FLX_LOCUS_TAIL
#define FLX_LOCUS_TAIL 3  // lanes without a known member behind the last one that has one, from which the span seeds again
#endif
// 8 waves per SIMD (63 registers instead of 68): 14.8 -> 14.3 ms per 1e10 positions; 9 and 10 are slower again (profiles/r04_microbench.txt)
#ifndef FLX_COVER_WAVES_PER_EU
#define FLX_COVER_WAVES_PER_EU 8
#endif
#define FLX_COVER_OCC __attribute__((amdgpu_waves_per_eu(FLX_COVER_WAVES_PER_EU, FLX_COVER_WAVES_PER_EU)))

// The 2-bit codes of the four bases of a dword (src/kmers.cpp:176-196: C/c 1, G/g 2, T/t 3, anything else 0) packed into 8
// bits, first base (lowest byte) in the top two.  Branch free (a switch per base compiles into divergent control flow — half
// of the cover kernel's run time once) and, since the cover kernel turned out to be bound by its vector instructions (round 4:
// 0.81 per position, a quarter of them here), by table: bits 1..3 of a letter tell A, C, T and G apart (0, 1, 2, 3 — in either
// case), v_perm_b32 looks up the letter that index stands for and the byte is that letter or it is none of them; a second
// v_perm_b32 turns the index into the code and v_dot4_u32_u8 packs the four.  12 instructions per dword (three SWAR comparisons: 30).
__device__ __forceinline__ uint32_t codes4(uint32_t w) {
    const uint32_t idx = (w >> 1) & 0x07070707u;
    const uint32_t letter = __builtin_amdgcn_perm(0u, 0x47544341u, idx);  // A C T G for 0 1 2 3, 0x00 for 4..7
    const uint32_t d = (letter ^ w) & 0xDFDFDFDFu;                         // a zero byte: that letter, upper or lower case
    const uint32_t nz = ((d & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | d;             // bit 7 of every byte that is NOT zero
    const uint32_t sel = ((nz >> 5) & 0x04040404u) | idx;                  // anything else: an index from 4 on
    const uint32_t code = __builtin_amdgcn_perm(0u, 0x02030100u, sel);     // A 0, C 1, T 3, G 2; 0 from 4 on
    return __builtin_amdgcn_udot4(code, 0x01041040u, 0u, false);           // byte 0 * 64 + byte 1 * 16 + byte 2 * 4 + byte 3
}

// The reverse complement of 16 bases in 2-bit codes (of a whole 32-base window, word by word: the canonical form of every prefilter
// pair's 11-mer is then one funnel shift — kmerset.h, flx_pre11).
__device__ __forceinline__ uint32_t rc32(uint32_t w) {
    const uint32_t r = __brev(w);
    return ~(((r >> 1) & 0x55555555u) | ((r & 0x55555555u) << 1));
}

// 16 bytes of the read plane.  The plane is streamed once and the coverage rows are written once: non-temporal, so that they do
// not push the prefilter out of the L2 (14.26 -> 13.8 ms per 1e10 positions, profiles/r04_microbench.txt)
__device__ __forceinline__ uint4 flx_plane16(const uint8_t *p) {
    const uint4 *q = reinterpret_cast<const uint4 *>(p);
    uint4 v;
    v.x = __builtin_nontemporal_load(&q->x); v.y = __builtin_nontemporal_load(&q->y);
    v.z = __builtin_nontemporal_load(&q->z); v.w = __builtin_nontemporal_load(&q->w);
    return v;
}
// A lane's left / right neighbour's value, with lane 0's / lane 63's coming from a wave-uniform carry: ONE DPP move (wave_shr:1 /
// wave_shl:1: a lane without a source keeps the destination's old value, which is set to the carry).  __shfl_up + `if (lane == 0)`
// compiles to ds_bpermute_b32 + v_cndmask_b32 with the lane mask held in an SGPR pair — twenty of those per span kept four such pairs
// alive in a kernel that is short of scalar registers (78 at 8 waves per SIMD: they were spilled to vector lanes and read back with
// two v_readlane each), and sent thirty operations per span through the LDS crossbar (round 5; tools/rejected/score_kmer_ablations.patch
// has the old form as FLX_COVER_NO_DPP).
__device__ __forceinline__ uint32_t flx_from_left(uint32_t x, uint32_t lane0) {
    return (uint32_t)__builtin_amdgcn_update_dpp((int)lane0, (int)x, 0x138 /* wave_shr:1 */, 0xf, 0xf, false);
}
__device__ __forceinline__ uint32_t flx_from_right(uint32_t x, uint32_t lane63) {
    return (uint32_t)__builtin_amdgcn_update_dpp((int)lane63, (int)x, 0x130 /* wave_shl:1 */, 0xf, 0xf, false);
}

struct CoverArgs {
    const uint8_t *plane;
    const uint64_t *offsets;
    const int32_t *lengths;
    const uint32_t *order;
    uint64_t n_reads;
    const uint8_t *exact15;
    const uint8_t *pre11;
    flx_locus loc;
    uint32_t *cov;
    const uint64_t *cov_off;
    int32_t *count, *first, *last;
    // k_kmer_cover_q: a mark per slot of the processing order — the reads the first kernel hands to the one with a diagonal per lane
    uint8_t *redo;
    // The cooperative path of long reads (cover_long.hip, cover_segments.h).  A batch launch leaves every read of at least long_min
    // bases alone (kCoverNoLong: none): nothing folded, nothing written, never marked.  A segment launch (template flag SEGMENTS)
    // runs on the segment table — offsets / lengths / cov_off / count / first / last / redo are the table's, one entry per virtual
    // read, `order` is NULL — and `emit` holds every segment's emit range in its virtual read's coordinates
    uint32_t long_min;
    const int2 *emit;
};
constexpr uint32_t kCoverNoLong = 0xffffffffu;
// (a pointer out of an integer: without the global address space on it every access would be a flat load with a 64-bit address
// built in vector registers — one more vector instruction per access)
#define FLX_GLOBAL_PTR(elem) const elem __attribute__((address_space(1))) *
#define FLX_KARG_PTR(elem, field) ((FLX_GLOBAL_PTR(elem))(uint64_t)(uintptr_t)(a.field))

// ---- a read of a launch ---------------------------------------------------------------------------------------------------------
// What a wave knows about its read before the first span (all wave-uniform).  SEGMENTS: a "read" is a virtual read [S, T) of a long
// read, its row starts at the word of base S in that read's row, and only the pieces inside its emit range (multiples of 32, or the
// virtual read's end) are written and counted.
struct CoverRead {
    uint32_t rid;
    int L;
    const uint8_t *seq;
    uint32_t *row;
    int row_words, n_spans;
    int emit_lo, emit_hi;
};
// false: a long read in a batch launch — covered in segments, the wave leaves it alone
template <bool SEGMENTS>
__device__ __forceinline__ bool cover_read(const CoverArgs &a, uint64_t slot, CoverRead &r) {
    r.rid = __builtin_amdgcn_readfirstlane(a.order ? a.order[slot] : (uint32_t)slot);
    r.L = __builtin_amdgcn_readfirstlane(a.lengths[r.rid]);
    if (!SEGMENTS && (uint32_t)r.L >= a.long_min) return false;
    r.seq = a.plane + a.offsets[r.rid];
    r.row = a.cov + (a.cov_off[r.rid] >> 2);
    r.row_words = (((r.L + 7) / 8 + 15) & ~15) >> 2;
    r.n_spans = (r.L + 1023) >> 10;
    r.emit_lo = r.emit_hi = 0;
    if (SEGMENTS) {
        const int2 er = a.emit[slot];
        r.emit_lo = __builtin_amdgcn_readfirstlane(er.x);
        r.emit_hi = __builtin_amdgcn_readfirstlane(er.y);
    }
    return true;
}
// Positions p0 + j (bit j) of a piece that begins inside the read which end a K-mer inside the read: K-mers end at K - 1 .. L - 1
// (all 16 of them except in the read's first and last piece)
__device__ __forceinline__ uint32_t piece_valid_mask(int p0, int L, int K) {
    uint32_t valid = 0xffffu;
    if (p0 < K - 1) valid &= ~((1u << (K - 1 - p0)) - 1u);
    if (p0 + 16 > L) valid &= (1u << (L - p0)) - 1u;
    return valid;
}

// ---- the text (kmerset.h: flx_locus) along a wave-uniform diagonal -----------------------------------------------------------------
struct LocusText {
    const CoverArgs &a;
    const int lane;
    const uint32_t n_alloc, seed_mask;
    const int seed_shift;
    const bool has_s1;
    __device__ __forceinline__ LocusText(const CoverArgs &args, int lane_)
        : a(args), lane(lane_), n_alloc(args.loc.n_alloc), seed_mask(args.loc.seed_mask), seed_shift(args.loc.seed_shift), has_s1(args.loc.safe1 != nullptr) {}
    // the index of the text word that holds the LAST base of the 16 that start at `base` + 16 * lane_off on the diagonal `dg` (clamped
    // into the padded array).  The diagonal and `base` are wave-uniform: the 64-bit part of the index is scalar work, a lane adds its
    // offset and clamps (the cover kernels are bound by their vector instructions)
    __device__ __forceinline__ uint32_t index(long long dg, int base, int lane_off) const {
        long long u = ((dg + base + 15) >> 4) + (long long)kLocusPad;  // (16 * lane + c) >> 4 == lane + (c >> 4)
        u = u < -64 ? -64 : (u > (long long)n_alloc ? (long long)n_alloc : u);
        const int w = (int)u + lane_off;
        return (uint32_t)max(0, min(w, (int)n_alloc - 1));
    }
    __device__ __forceinline__ uint2 word_at(uint32_t i) const {
        // (a 32-bit byte offset on a scalar base: one address register — the text has at most 2^28 positions, 2^27 bytes.  Non-temporal
        // here is slower: 14.2 vs 13.8 ms per 1e10 — a text word is used again by the next span's lane 0 and by reads of the same locus)
        const uint64_t tv = *(FLX_GLOBAL_PTR(uint64_t))(FLX_KARG_PTR(uint8_t, loc.text) + (uint32_t)(i * 8u));
        return make_uint2((uint32_t)tv, (uint32_t)(tv >> 32));
    }
    __device__ __forceinline__ uint32_t safe_at(uint32_t i) const {  // the S1 bits of that word (kmerset.h: safe1)
        return has_s1 ? (uint32_t)*(FLX_GLOBAL_PTR(uint16_t))(FLX_KARG_PTR(uint8_t, loc.safe1) + (uint32_t)(i * 2u)) : 0u;
    }
    // this lane's word of the span whose first base is `base`
    __device__ __forceinline__ uint2 word(long long dg, int base) const { return word_at(index(dg, base, lane)); }
    __device__ __forceinline__ uint32_t safe(long long dg, int base) const { return safe_at(index(dg, base, lane)); }
    // the seed table: the text position of the 16 bases `lo` (hash, four linear probes), or kLocusEmpty
    __device__ __forceinline__ uint32_t seed(uint32_t lo) const {
        uint32_t h = flx_locus_hash(lo, seed_shift);
        FLX_GLOBAL_PTR(uint32_t) seed_tab = FLX_KARG_PTR(uint32_t, loc.seed);
        FLX_GLOBAL_PTR(uint32_t) seed_text = FLX_KARG_PTR(uint32_t, loc.text);  // (.x of text word i at dword 2 i)
#pragma unroll 1
        for (int probe_no = 0; probe_no < 4; ++probe_no) {
            const uint32_t v = seed_tab[h];
            if (v == kLocusEmpty) break;
            {  // (flx_locus_kmer_at, kmerset.h, on the global-space pointer)
                const uint32_t tw_i = (v >> 4) + kLocusPad, ts_i = v & 15u;
                const uint32_t t0 = seed_text[2 * tw_i];
                const uint32_t at = ts_i == 0 ? t0 : __builtin_amdgcn_alignbit(t0, seed_text[2 * tw_i + 2], 32 - 2 * ts_i);
                if (at == lo) return v;
            }
            h = (h + 1) & seed_mask;
        }
        return kLocusEmpty;
    }
};

// The 2-bit XOR of 16 bases with the text's -> bit j: base j differs (base 0 = the earliest, which sits in the top two bits)
__device__ __forceinline__ uint32_t mismatch16(uint32_t x) {
    uint32_t m = (x | (x >> 1)) & 0x55555555u;  // even bit 2k: the base k places from the END differs
    m = (m | (m >> 1)) & 0x33333333u;
    m = (m | (m >> 2)) & 0x0f0f0f0fu;
    m = (m | (m >> 4)) & 0x00ff00ffu;
    m = (m | (m >> 8)) & 0xffffu;
    return __brev(m) >> 16;
}

// ---- the text verdict ----------------------------------------------------------------------------------------------------------------
// What the text at one place says about a piece.  The window is 32 bases: the 16 in front of the piece's own (bits 0 .. 15) and its
// own (bits 16 .. 31).  z: bit i = base i matches the text; b32 / u32 / s32: the text's flags under base i — the first base of a piece
// of the text, the start of a 13-mer that occurs nowhere else in it (U13, only set inside one piece), the 16 bases from i on are S1
// (no 16-mer one base away from the text's is a member).  All of it is about the TEXT at that place and true whatever the read's real
// locus is.  Bit j of an answer is the piece's position j:
//   known    (added to) the 16-mer ending there matches the text inside one piece: it IS a member;
//   text12   (added to) the 12 bases ending there match the text inside one piece: that 12-mer IS present;
//   returns  refuted: not a text match, but holds a text-matching U13 13-mer, or differs from an S1 text window in exactly one base:
//            it is NOT a member.  (Returned, not added: a caller that knows nothing about the bases in front of a lane cuts it first.)
// any_start = false (wave-uniform; b32 == 0): no piece start in sight, every window lies inside one piece — piece starts are rare, two
// per contig, and the masks that keep a window inside one piece are 25 of the comparison's ~100 instructions.
__device__ __forceinline__ uint32_t text_verdict(uint32_t z, uint32_t b32, uint32_t u32, uint32_t s32, uint32_t valid16, bool any_start, uint32_t &known, uint32_t &text12) {
    uint32_t r = z & (z >> 1);
    r &= r >> 2;
    r &= r >> 4;
    r &= r >> 8;  // bit i: bases i .. i + 15 match
    uint32_t q = 0xffffffffu, q12 = 0xffffffffu;
    if (any_start) {
        q = ~b32 >> 1;  // bit i: no piece starts at base i + 1
        q &= q >> 1;
        q &= q >> 2;
        q &= q >> 4;
        q &= q >> 7;  // bit i: none at i + 1 .. i + 15 — the 16 bases from i on lie in one piece of the text
        q12 = ~b32 >> 1;
        q12 &= q12 >> 1;
        q12 &= q12 >> 2;
        q12 &= q12 >> 4;
        q12 &= q12 >> 3;  // bit i: no piece starts at i + 1 .. i + 11 (a piece has at least 16 bases: the 12-mer lies in one of its 16-mers)
    }
    {
        uint32_t m12 = z & (z >> 1);
        m12 &= m12 >> 2;
        m12 &= m12 >> 4;
        m12 &= m12 >> 4;  // bit i: bases i .. i + 11 match
        text12 |= ((m12 & q12) >> 5) & 0xffffu;  // the 12-mer ending at position j starts at base j + 5
    }
    r &= q;
    known |= (r >> 1) & valid16;  // the 16-mer ending at position j starts at base j + 1 of the window
    uint32_t g = z & (z >> 1);
    g &= g >> 2;
    g &= g >> 4;
    g &= g >> 5;  // bit i: bases i .. i + 12 match the text
    g &= u32;     // ... and that 13-mer occurs nowhere else
    g |= g >> 1;
    g |= g >> 2;  // bit i: such a 13-mer starts at base i, i + 1, i + 2 or i + 3: inside the 16 bases from i on
    // S1: exactly ONE of the 16 bases from i on differs from the text (counted with a saturating two-bit counter per window: `one` =
    // exactly one mismatch, `two` = more)
    uint32_t one = ~z, two;
    two = one & (one >> 1);
    one ^= one >> 1;
    {
        const uint32_t t2 = two | (two >> 2) | (one & (one >> 2));
        one = (one ^ (one >> 2)) & ~t2;
        two = t2;
    }
    {
        const uint32_t t2 = two | (two >> 4) | (one & (one >> 4));
        one = (one ^ (one >> 4)) & ~t2;
        two = t2;
    }
    {
        const uint32_t t2 = two | (two >> 8) | (one & (one >> 8));
        one = (one ^ (one >> 8)) & ~t2;
    }
    one &= q & s32;
    return (((g & ~r) | one) >> 1) & valid16;
}

// ---- the 12-mer prefilter: one pair of positions ---------------------------------------------------------------------------------------
// x13 = x.C.y, the 13 bases that end at the pair's second position (low 26 bits), rc22 = the reverse complement of C.  The byte of
// pre11 (kmerset.h, flx_pre11) that answers both positions, and the two answers out of it.  Where the middle base of C is G or T the
// byte belongs to the other strand and is looked at bit-reversed — bit 7 - x is bit x, bit 3 - y is bit 4 + y — instead of with two
// selected bit numbers: 19 instead of 33 instructions per pair.
__device__ __forceinline__ uint32_t pre11_pair_index(uint32_t x13, uint32_t rc22) {
    const uint32_t kk = (x13 & 0x2000u) ? rc22 : ((x13 >> 2) & 0x3FFFFFu);
    return ((kk >> 12) << 11) | (kk & 0x7FFu);
}
__device__ __forceinline__ uint32_t pre11_pair_bits(uint32_t x13, uint32_t byte) {
    const uint32_t b = (x13 & 0x2000u) ? (__brev(byte) >> 24) : byte;
    return ((b >> ((x13 >> 24) & 3u)) & 1u) | (((b >> (4u + (x13 & 3u))) & 1u) << 1);
}

// ---- exact membership and the outermost-member search ------------------------------------------------------------------------------------
// One byte of exact15 answers the pair of positions (a, a + 1), any a in 0..14 — the 15 bases ending at a are the byte's index, the
// base before them picks the bit of position a, the base after them the bit of a + 1.  A question from ABOVE (top-down search) takes
// the pair that ENDS at the asked position, one from below the pair that starts there: either way the request also settles the next
// candidate in the direction of the search.  top / bot: the positions asked from above / from below, -1 = none; `keep` cuts the
// answers (positions outside the read hold no 16-mer).
// Plain byte loads: non-temporal ones measured 8 % slower here (43.3 vs 40.1 ms per 1e10 positions), 4-byte loads 6 % slower —
// although a microbenchmark that mixes table and far lookups in one burst prefers nt (tools/tabench (7)).
__device__ __forceinline__ void exact_pair_probe(const CoverArgs &a, uint32_t hi, uint32_t lo, int top, int bot, uint32_t keep, uint32_t &hits, uint32_t &probed) {
    const int a0 = top > 0 ? top - 1 : 0, a1 = bot < 14 ? bot : 14;
    uint32_t g0 = 0, g1 = 0;
    FLX_GLOBAL_PTR(uint8_t) exact15 = FLX_KARG_PTR(uint8_t, exact15);
    if (top >= 0) g0 = exact15[__builtin_amdgcn_alignbit(hi, lo, 30 - 2 * a0) & 0x3FFFFFFFu];
    if (bot >= 0) g1 = exact15[__builtin_amdgcn_alignbit(hi, lo, 30 - 2 * a1) & 0x3FFFFFFFu];
    if (top >= 0) {
        const uint32_t x = (hi >> (28 - 2 * a0)) & 3u, y = (lo >> (28 - 2 * a0)) & 3u;
        hits |= (((g0 >> x) & 1u) | (((g0 >> (4 + y)) & 1u) << 1)) << a0;
        probed |= 3u << a0;
    }
    if (bot >= 0) {
        const uint32_t x = (hi >> (28 - 2 * a1)) & 3u, y = (lo >> (28 - 2 * a1)) & 3u;
        hits |= (((g1 >> x) & 1u) | (((g1 >> (4 + y)) & 1u) << 1)) << a1;
        probed |= 3u << a1;
    }
    hits &= keep;
}
// One step of the search in a piece's window of 17 positions (bit 0 = the left neighbour's last position, bit j + 1 = position j): the
// highest open candidate above the confirmed members and the lowest one below them.  A base is covered iff ANY 16-mer over it is a
// member, and two confirmed members inside the window are at most 16 apart, so only the OUTERMOST members matter.  false: nothing to ask
__device__ __forceinline__ bool next_asks(uint32_t cand, uint32_t hits, uint32_t probed, uint32_t left_member, int &top, int &bot) {
    const uint32_t H = (hits << 1) | left_member;
    const uint32_t open = (cand & ~probed) << 1;
    uint32_t above = open, below = open;
    if (H) {
        above = open & ~((2u << (31 - __clz(H))) - 1u);
        below = open & ((H & (0u - H)) - 1u);
    }
    top = above ? 30 - __clz(above) : -1;  // position = bit - 1
    bot = below ? __ffs(below) - 2 : -1;
    if (bot >= 0 && bot + 1 >= top && top >= 0) bot = -1;  // the two questions meet: the pair that ends at `top` answers both
    return (top & bot) != -1;
}

// ---- hits -> coverage ------------------------------------------------------------------------------------------------------------------
// The 16 coverage bits of a piece out of its hits and its right neighbour's: bit j = OR of hit bits j .. j + 15 — base p0 + j lies in a
// member 16-mer (src/read.cpp:53-54)
__device__ __forceinline__ uint32_t dilate16(uint32_t h, uint32_t next) {
    uint32_t x = h | (next << 16);
    x |= x >> 1;
    x |= x >> 2;
    x |= x >> 4;
    x |= x >> 8;
    return x & 0xffffu;
}
// ... without the positions behind the read's end
__device__ __forceinline__ uint32_t cut_tail16(uint32_t c16, int p0, int L) {
    if (p0 >= L) return 0;
    if (p0 + 16 > L) c16 &= (1u << (L - p0)) - 1u;
    return c16;
}
// covered count / first covered base / one past the last (m_first_base_in_kmer / m_last_base_in_kmer, src/read.cpp:75-84)
struct CoverTally {
    int cnt = 0, fst = 0x7fffffff, lst = -1;
    __device__ __forceinline__ void add(uint32_t c16, int p0) {
        cnt += __popc(c16);
        if (c16) {
            fst = min(fst, p0 + (__ffs(c16) - 1));
            lst = max(lst, p0 + (32 - __clz(c16)));
        }
    }
    __device__ __forceinline__ void reduce_wave() {
        for (int o = 32; o > 0; o >>= 1) {
            cnt += __shfl_xor(cnt, o, 64);
            fst = min(fst, __shfl_xor(fst, o, 64));
            lst = max(lst, __shfl_xor(lst, o, 64));
        }
    }
    __device__ __forceinline__ void store(uint32_t rid, int32_t *count, int32_t *first, int32_t *last) const {
        count[rid] = cnt;
        first[rid] = cnt ? fst : -1;
        last[rid] = cnt ? lst : -1;
    }
};
// A lane's piece of span sp of a wave-level kernel: h = its hits, next = its right neighbour's -> coverage bits, counts, row word
// (non-temporal: cover rows are written once)
template <bool SEGMENTS>
__device__ __forceinline__ void emit_piece(const CoverRead &r, int sp, int lane, uint32_t h, uint32_t next, CoverTally &t) {
    const int p0 = (sp << 10) + lane * 16;
    uint32_t c16 = dilate16(h, next);
    if (((sp + 1) << 10) > r.L) c16 = cut_tail16(c16, p0, r.L);  // (wave-uniform: only the read's last span has positions to cut off)
    const bool emitted = !SEGMENTS || (p0 >= r.emit_lo && p0 < r.emit_hi);  // (a piece lies inside the emit range or outside it)
    if (!emitted) c16 = 0;
    t.add(c16, p0);
    const uint32_t up = flx_from_right(c16, 0u);  // (only the even lanes write: lane 63's is never used)
    const int word = p0 >> 5;
    if ((lane & 1) == 0 && (SEGMENTS ? emitted : word < r.row_words)) __builtin_nontemporal_store(c16 | (up << 16), &r.row[(uint32_t)word]);
}
// The end of a read in a wave-level kernel: the padding words of its row (rows are padded to 16 bytes; only L == 0 leaves words
// unwritten), then count / first / last (SEGMENTS: the segment's, in its virtual read's coordinates — flx_cover_long_reduce)
template <bool SEGMENTS>
__device__ __forceinline__ void wave_reduce_and_store(const CoverArgs &a, const CoverRead &r, int lane, CoverTally &t) {
    if (!SEGMENTS)
        for (int wd = r.n_spans * 32 + lane; wd < r.row_words; wd += 64) r.row[wd] = 0;
    t.reduce_wave();
    if (lane == 0) t.store(r.rid, a.count, a.first, a.last);
}

// cover_queue.hip: the cover kernel of round 6 (sets with a text); returns a HIP launch error through the context
// (every_read_to_second: FLX_KMER_COVER=q2, tests — every read goes straight to the kernel with a diagonal per lane)
// (segments: args name a segment table — the kernels' SEGMENTS instantiations)
int flx_cover_queue_launch(flx_ctx *ctx, const CoverArgs &args, bool has_prefilter, unsigned grid, bool every_read_to_second, bool segments = false);

// ---- cover_long.hip: the cooperative path of the coverage stage — long reads covered as segments, one wave each ----
struct CoverLongCounts {  // counted by k_cov_row_bytes, read back with the coverage plane's size; the cursors serve the table kernel
    unsigned long long n_reads, n_segs, read_cursor, seg_cursor;
};
struct CoverLong {
    bool on = false;  // the path applies to this call
    int thr = 0;      // reads of at least thr bases are covered in segments
    int spans = 0;    // spans (1024 bases) per segment
    CoverLongCounts n = {0, 0, 0, 0};
    double t_start = 0.0;
};
// FLX_KMER_COVER_LONG_MIN / FLX_KMER_COVER_LONG_SPANS and the default rule -> cl (an invalid value of either switch: FLX_ERR_INVALID)
int flx_cover_long_threshold(flx_ctx *ctx, uint64_t plane_bytes, bool applies, CoverLong *cl);
size_t flx_cover_long_workspace(const CoverLongCounts &n);
// builds the segment table in `work` (stream-ordered) and turns the batch's arguments into the segment launch's
int flx_cover_long_table(flx_ctx *ctx, CoverLong &cl, const CoverArgs &batch, CoverLongCounts *d_counts, void *work, size_t work_bytes, CoverArgs *seg);
// after the segment launch: every long read's count / first / last out of its segments', and the padding words of its row
int flx_cover_long_reduce(flx_ctx *ctx, const CoverLong &cl, const CoverArgs &batch, void *work);
// FLX_API_TIMING: the stage line (after the wait that ends the call's device work)
void flx_cover_long_report(const CoverLong &cl);

// ---- the stage (cover_wave.hip) ----------------------------------------------------------------------------------------------------------
// FLX_KMER_COVER=v2, or a set without the pair table (finalize found no room for it): the workgroup-per-read kernel covers the call
bool flx_kmer_cover_is_v2(const flx_kmerset *set);
// Lookups -> coverage bits: the rows of `cov` and count / first / last of every read.  Chooses the form (FLX_KMER_COVER,
// FLX_KMER_LOCUS; ctx->last_kmer_cover / _locus / _redo say which ran), launches it on the batch and — cvl.n.n_segs — on the segment
// table of the batch's long reads built in long_work.  Timing brackets: flx_score_kmer_cover, flx_score_kmer_cover.long.
int flx_kmer_cover_stage(flx_ctx *ctx, const flx_kmerset *set, const uint8_t *d_plane, const uint64_t *d_offsets, const int32_t *d_lengths, const uint32_t *d_order,
                         uint64_t n_reads, uint32_t *d_cov, const uint64_t *d_covoff, int32_t *d_count, int32_t *d_first, int32_t *d_last, uint8_t *d_redo,
                         CoverLong &cvl, CoverLongCounts *d_long_counts, void *long_work, size_t long_work_bytes);
