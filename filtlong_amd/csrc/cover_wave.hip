// cover_wave.hip — the coverage stage of k-mer mode: its host entry (flx_kmer_cover_stage) and the two kernels that need no queue.
//
// Reference semantics: the k-mer branch of Read::Read, src/read.cpp:43-58 — a rolling 2-bit 16-mer, one set lookup per position,
// bases i-15..i marked on a hit; here: seq plane -> coverage bit plane (1 bit per base) + covered count / first / last covered base
// per read (src/read.cpp:75-84).  The qualities of k-mer mode are 0.0 / 1.0, so the reference's serial FP64 sum is an exact integer:
// mean = 100 * popcount / L needs no serial pass; the window folds over the bits are score_kmer.hip's.
//   k_kmer_cover    one workgroup per read (round 2, "v2"): what a set without the pair table runs, and FLX_KMER_COVER=v2
//   k_kmer_cover_w  one wavefront per read (rounds 3-5): what a set without a text runs, and FLX_KMER_COVER=w
// The default for a set with a text is k_kmer_cover_q (cover_queue.hip); long reads go through either wave-level kernel as segments
// (cover_long.hip).  What the three share — every rule of the filter — is in cover_common.h.
#include "flx_internal.h"
#include "kmerset.h"
#include "cover_common.h"

#ifndef FLX_FARFIRST_LANES
#define FLX_FARFIRST_LANES 16  // settled lanes of a span from which the next span asks the exact table first (k_kmer_cover_w, below)
#endif
#ifndef FLX_FARFIRST_LANES_LOCUS
#define FLX_FARFIRST_LANES_LOCUS 65  // the same with a text: never (65 > 64) — the text settles the clean lanes, the mode only costs instructions (profiles/r04_microbench.txt)
#endif

namespace {

// ---------------------------------------------------------------------------------------------------
// coverage
// ---------------------------------------------------------------------------------------------------
// One workgroup per read, COVER_THREADS * 16 positions per iteration.  Two instantiations share the batch: 256 threads
// (spans of 4096 positions) for reads longer than kCoverShort, one wavefront (spans of 1024) for the short ones, which
// would leave most of a 256-thread workgroup idle (500 bp reads: 206 -> 98 ms per 1e10 bases, 2 kbp: 83 -> 71; profiles/r02_microbench.txt).
constexpr int kCoverShort = 3072;

template <int COVER_THREADS>
__global__ void __launch_bounds__(COVER_THREADS) k_kmer_cover(const uint8_t *plane, const uint64_t *offsets,
                                                              const int32_t *lengths, const uint32_t *order,
                                                              uint64_t n_reads, const uint32_t *bitmap,
                                                              const uint32_t *prefilter, uint32_t *cov, const uint64_t *cov_off, int32_t *count,
                                                              int32_t *first, int32_t *last) {
    constexpr int COVER_SPAN = COVER_THREADS * 16;  // positions per workgroup iteration
    __shared__ uint32_t sh_hits[COVER_THREADS];
    __shared__ uint16_t sh_p12[COVER_THREADS];
    __shared__ uint8_t sh_anchor[COVER_THREADS];
    __shared__ uint32_t sh_carry;
    __shared__ int sh_cnt[COVER_THREADS / 64], sh_first[COVER_THREADS / 64], sh_last[COVER_THREADS / 64];
    for (uint64_t slot = blockIdx.x; slot < n_reads; slot += gridDim.x) {
        const uint32_t rid = order ? order[slot] : (uint32_t)slot;
        const int L = lengths[rid];
        if ((L > kCoverShort) != (COVER_THREADS > 64)) continue;  // the other instantiation's read (uniform for the workgroup)
        const uint8_t *seq = plane + offsets[rid];
        uint32_t *row = cov + (cov_off[rid] >> 2);
        const int row_words = (((L + 7) / 8 + 15) & ~15) >> 2;
        const int t = threadIdx.x;
        CoverTally tally;
        if (t == 0) sh_carry = 0;
        __syncthreads();
        const int n_spans = (L + COVER_SPAN - 1) / COVER_SPAN;
        for (int sp = n_spans - 1; sp >= 0; --sp) {  // descending: the right neighbour's hits are already known
            const int p0 = sp * COVER_SPAN + t * 16;
            const bool active = p0 < L && L >= 16;
            uint32_t hits = 0;
            uint32_t kmers[16];
            uint32_t kleft[5] = {0, 0, 0, 0, 0};  // the 16-mers ending at p0-5 .. p0-1 (their low 24 bits are the 12-mers there)
            uint32_t p12 = 0;                     // bit j: the 12-mer ending at p0 + j occurs in the set
            uint32_t p12_left = 0;                // the same for p0-5 .. p0-1 (only the first thread of a span looks them up itself)
            if (active) {
                // bases [p0-16, p0+16): both loads are 16-byte aligned (read starts are)
                uint4 a = make_uint4(0, 0, 0, 0);
                if (p0 > 0) a = *reinterpret_cast<const uint4 *>(seq + p0 - 16);
                const uint4 b = *reinterpret_cast<const uint4 *>(seq + p0);
                // 2 bits per base: hi = bases p0-16 .. p0-1, lo = bases p0 .. p0+15 (earliest base in the top bits); the 16-mer
                // ending at p0 + j is a 32-bit window of hi:lo
                const uint32_t hi = (codes4(a.x) << 24) | (codes4(a.y) << 16) | (codes4(a.z) << 8) | codes4(a.w);
                const uint32_t lo = (codes4(b.x) << 24) | (codes4(b.y) << 16) | (codes4(b.z) << 8) | codes4(b.w);
#pragma unroll
                for (int j = 0; j < 15; ++j) kmers[j] = __builtin_amdgcn_alignbit(hi, lo, 2 * (15 - j));
                kmers[15] = lo;
#pragma unroll
                for (int j = 0; j < 5; ++j) kleft[j] = hi >> (2 * (4 - j));  // low 24 bits: the 12-mer ending at p0 - 5 + j
                // 12-mer prefilter (kmerset.h): one L2 lookup per position, all 16 in flight
                if (prefilter) {
                    uint32_t pw[16];
#pragma unroll
                    for (int j = 0; j < 16; ++j) pw[j] = prefilter[flx_sub12(kmers[j], 0) >> 5];
#pragma unroll
                    for (int j = 0; j < 16; ++j) {
                        const int i = p0 + j;
                        if (i >= 11 && i < L) p12 |= ((pw[j] >> (kmers[j] & 31)) & 1u) << j;
                    }
                    if (t == 0 && p0 > 0) {
#pragma unroll
                        for (int j = 0; j < 5; ++j)
                            if (p0 - 5 + j >= 11) p12_left |= ((prefilter[flx_sub12(kleft[j], 0) >> 5] >> (kleft[j] & 31)) & 1u) << j;
                    }
                } else {
                    p12 = 0xffffu;
                    p12_left = 0x1fu;
                }
            }
            sh_p12[t] = (uint16_t)p12;
            __syncthreads();
            // Candidates: bit j = the 16-mer ending at p0 + j may be present (all five of its 12-mers are, and it lies in the read).
            // Lookups: a base is covered iff ANY 16-mer over it is present, so of a run of consecutive candidates only
            // the END points matter as long as they are present — their spans [j-15, j] overlap inside a thread's 16
            // positions and cover everything the run's other members could.  Per thread: probe the first and last
            // candidate of every run (the first one is skipped when the run continues from the left neighbour and that
            // neighbour's last probe hit); only if a probe MISSES (a filter false positive, ~2 %) are the run's other
            // members looked up too.  Coverage is identical to looking all of them up; far requests per position drop
            // from one per present 16-mer to ~2 per clean stretch.
            uint32_t cand = 0, probed = 0;
            bool left_run = false;  // the candidate run at bit 0 continues from the left neighbour's bit 15
            if (active) {
                if (t > 0) p12_left = prefilter ? (uint32_t)(sh_p12[t - 1] >> 11) : 0x1fu;
                const uint32_t m = (p12_left >> 1) | (p12 << 4);  // bit i: the 12-mer ending at p0 - 4 + i
                cand = m & (m >> 1) & (m >> 2) & (m >> 3) & (m >> 4) & 0xffffu;
                cand &= piece_valid_mask(p0, L, 16);
                left_run = t > 0 && p12_left == 0x1fu && p0 - 1 >= 15;  // the left neighbour's bit 15 is a candidate
                const uint32_t starts = cand & ~(cand << 1), ends = cand & ~(cand >> 1);
                probed = ends | (left_run ? starts & ~1u : starts);
                uint32_t words[16];
#pragma unroll
                for (int j = 0; j < 16; ++j) words[j] = ((probed >> j) & 1u) ? bitmap[kmers[j] >> 5] : 0u;  // independent, in flight
#pragma unroll
                for (int j = 0; j < 16; ++j)
                    if ((probed >> j) & 1u) hits |= ((words[j] >> (kmers[j] & 31)) & 1u) << j;
            }
            sh_anchor[t] = (uint8_t)((hits >> 15) & 1u);
            __syncthreads();
            if (active) {
                if ((cand & 1u) && !(probed & 1u)) {  // run continuing from the left: its start is needed only if the neighbour's end missed
                    if (!sh_anchor[t - 1]) {
                        probed |= 1u;
                        hits |= (bitmap[kmers[0] >> 5] >> (kmers[0] & 31)) & 1u;
                    }
                }
                // A probe that missed (typically a false candidate right behind a clean stretch: the 12-mers it shares with the
                // stretch are genuine, so the filter passes it with probability ~0.45): what is still needed for an exact answer
                // are the run members OUTSIDE the span of its confirmed ones (or all of it, if none is confirmed yet).  Round 2
                // asks for those within 4 positions of a missed probe (a false extension is rarely longer), round 3 for the rest.
                auto still_needed = [&]() -> uint32_t {
                    uint32_t up = hits, dn = hits, m = cand;  // flood the confirmed bits along their candidate runs
                    up |= (up << 1) & m; dn |= (dn >> 1) & m;
                    uint32_t mu = m & (m << 1), md = m & (m >> 1);
                    up |= (up << 2) & mu; dn |= (dn >> 2) & md;
                    mu &= mu << 2; md &= md >> 2;
                    up |= (up << 4) & mu; dn |= (dn >> 4) & md;
                    mu &= mu << 4; md &= md >> 4;
                    up |= (up << 8) & mu; dn |= (dn >> 8) & md;
                    const uint32_t inside = up & dn;  // between the lowest and the highest confirmed member of a run
                    return cand & ~inside & ~probed & 0xffffu;
                };
                if (probed & ~hits) {
                    const uint32_t miss = probed & ~hits;
                    uint32_t near = (miss << 1) | (miss << 2) | (miss << 3) | (miss << 4) | (miss >> 1) | (miss >> 2) | (miss >> 3) | (miss >> 4);
                    for (int round = 0; round < 2; ++round) {
                        const uint32_t ask = still_needed() & (round == 0 ? near : 0xffffu);
                        if (ask) {
                            uint32_t words[16];
#pragma unroll
                            for (int j = 0; j < 16; ++j) words[j] = ((ask >> j) & 1u) ? bitmap[kmers[j] >> 5] : 0u;
#pragma unroll
                            for (int j = 0; j < 16; ++j)
                                if ((ask >> j) & 1u) hits |= ((words[j] >> (kmers[j] & 31)) & 1u) << j;
                            probed |= ask;
                        }
                    }
                }
            }
            sh_hits[t] = hits;
            __syncthreads();
            const uint32_t next = (t + 1 < COVER_THREADS) ? sh_hits[t + 1] : sh_carry;
            const uint32_t c16 = cut_tail16(dilate16(hits, next), p0, L);
            tally.add(c16, p0);
            const uint32_t hi = __shfl_down(c16, 1, 64);
            const int word = p0 >> 5;
            if ((t & 1) == 0 && word < row_words) row[word] = c16 | (hi << 16);
            __syncthreads();
            if (t == 0) sh_carry = hits;
            __syncthreads();
        }
        // zero the padding words beyond the spans (rows are padded to 16 bytes)
        for (int wd = n_spans * (COVER_SPAN / 32) + t; wd < row_words; wd += COVER_THREADS) row[wd] = 0;
        // block reduction of count / first / last
        tally.reduce_wave();
        if ((t & 63) == 0) {
            sh_cnt[t >> 6] = tally.cnt;
            sh_first[t >> 6] = tally.fst;
            sh_last[t >> 6] = tally.lst;
        }
        __syncthreads();
        if (t == 0) {
            CoverTally all;
            for (int wv = 0; wv < COVER_THREADS / 64; ++wv) {
                all.cnt += sh_cnt[wv];
                all.fst = min(all.fst, sh_first[wv]);
                all.lst = max(all.lst, sh_last[wv]);
            }
            all.store(rid, count, first, last);
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------------
// coverage, wave level (round 3) — the kernel that runs; k_kmer_cover above stays as the second implementation
// (FLX_KMER_COVER=v2, cross-checked in the tests)
// ---------------------------------------------------------------------------------------------------
// One WAVEFRONT owns a read and walks it left to right in spans of 1024 positions; a lane owns 16 consecutive positions
// (one 16-byte load, prefetched one span ahead).  No LDS, no barrier: the left neighbour's bases / 12-mer bits / last
// candidate travel by __shfl_up, lane 63's by a wave-uniform carry into the next span, and the coverage of a span is
// written one span late, when the hits of its right neighbour are known.
//
// What a lookup costs (tools/tabench, profiles/r03_microbench.txt): one distinct cache LINE per instruction — 261 G/s
// from the L2, 55 G/s beyond it, the two classes add up — so the kernel is built around lines, not lanes:
//   * prefilter: ONE byte of `pre11` answers the 12-mers of two consecutive positions (kmerset.h): 8 loads per lane;
//   * exact membership: ONE byte of `exact15` answers the 16-mers of two consecutive positions: a far request per PAIR;
//   * which pairs are asked: a base is covered iff ANY 16-mer over it is a member, and two confirmed members inside a
//     lane's window of 17 positions (its own 16 + the left neighbour's last) are at most 16 apart, so together they cover
//     everything a candidate between them could.  Only the OUTERMOST members matter: search the candidates from the top
//     down until the first member, and from the bottom up (not at all if the left neighbour's last position is a member),
//     one pair per side and round; a clean stretch costs one request per 16 positions, a false candidate costs one only
//     when it lies outside the confirmed span.  Rounds repeat until no lane of the wave has an open question.
//
// LOCUS (round 4, assembly references — kmerset.h: flx_locus): the wave carries a DIAGONAL, the text position its read's base 0
// would have in the assembly.  Every lane compares its 16 bases with the text along the diagonal (one coalesced 8-byte load per
// lane and span, prefetched a span ahead); 16 matching bases inside one strand copy ARE a member, without any request — `known`.
// The known members enter the search as confirmed hits: a lane whose own last 16-mer and whose left neighbour's are known is
// settled before anything is asked, a lane with a mismatch looks up only the prefilter pairs outside [lowest hit - 4, highest
// hit] and asks the exact table only outside its confirmed span, exactly as before (a 16-mer with a mismatch against the locus
// may still occur elsewhere).  The diagonal comes from the seed table: eight lanes look their own 16 bases up (one far request
// each) when the wave has none or the last 16 lanes of the previous span matched nowhere; a seed that fails leaves the old
// diagonal in place as a hypothesis that costs nothing to test.
// SEGMENTS: the launch on the segment table of the batch's long reads (cover_long.hip), as in k_kmer_cover_q.
template <bool HAS_PREFILTER, bool LOCUS, bool SEGMENTS = false>
__global__ void __launch_bounds__(FLX_COVER_THREADS) FLX_COVER_OCC k_kmer_cover_w(const CoverArgs a) {
    const int lane = threadIdx.x & 63;
    const uint64_t wave0 = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint64_t n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    const LocusText text(a, lane);
    for (uint64_t slot = wave0; slot < a.n_reads; slot += n_waves) {
        CoverRead rd;
        if (!cover_read<SEGMENTS>(a, slot, rd)) continue;
        const int L = rd.L, n_spans = rd.n_spans;
        CoverTally tally;
        // carried from lane 63 of the previous span (wave-uniform)
        uint32_t c_lo = 0, c_p12 = 0, c_cand15 = 0, c_hit15 = 0;
        uint32_t prev_hits = 0;  // hits of the previous span, waiting for their right neighbour's
        bool far_first = false;  // this span asks the exact table BEFORE the prefilter (decided by the previous span, below)
        // LOCUS: the diagonal (wave-uniform), whether a seed is due, the text of this span / the next one, lane 63's carry
        long long diag = 0;
        bool have_diag = false, carry_ok = false;
        uint32_t c_mb = 0xffffffffu /* mismatches | piece starts << 16 of lane 63 */, c_us = 0 /* its U13 | S1 << 16 */, c_known15 = 0, c_twx = 0, c_twy = 0xffffu;
        uint2 tw = make_uint2(0, 0xffffu), tw_next = make_uint2(0, 0xffffu);
        uint32_t ts = 0, ts_next = 0, c_ts = 0;  // S1 bits of those text words (kmerset.h: safe1); lane 63's for the next span
        uint4 raw = make_uint4(0, 0, 0, 0);
        // (offsets as unsigned 32-bit values: a uniform base plus a 32-bit lane offset is one address register, not two)
        if (lane * 16 < L) raw = flx_plane16(rd.seq + (uint32_t)(lane * 16));  // rows are 16-byte aligned and padded
        for (int sp = 0; sp < n_spans; ++sp) {
            const int p0 = (sp << 10) + lane * 16;
            uint4 raw_next = make_uint4(0, 0, 0, 0);
            if (p0 + 1024 < L) raw_next = flx_plane16(rd.seq + (uint32_t)(p0 + 1024));
            if (LOCUS && have_diag && sp + 1 < n_spans) {
                tw_next = text.word(diag, (sp << 10) + 1024);
                ts_next = text.safe(diag, (sp << 10) + 1024);
            }
            // 2 bits per base, earliest base on top: lo = my 16 bases, hi = the 16 before them
            const uint32_t lo = (codes4(raw.x) << 24) | (codes4(raw.y) << 16) | (codes4(raw.z) << 8) | codes4(raw.w);
            const uint32_t hi = flx_from_left(lo, c_lo);
            // positions p0 + j that end a 12-mer / a 16-mer inside the read
            uint32_t valid12 = 0, valid16 = 0;
            if (sp > 0 && ((sp + 1) << 10) <= L) {  // (wave-uniform: a span inside the read has every position, no lane computes masks)
                valid12 = valid16 = 0xffffu;
            } else if (p0 < L) {
                valid12 = piece_valid_mask(p0, L, 12);
                valid16 = piece_valid_mask(p0, L, 16);
            }
            // ---- LOCUS: members known from the text along the diagonal ----
            uint32_t known = 0, refuted = 0;  // refuted: not a text match, but holds a text-matching 13-mer that occurs nowhere else
            uint32_t text12 = 0;              // bit j: the 12 bases ending at my position j match the text inside one piece: that 12-mer IS present
            if (LOCUS) {
                // my 16 bases against the text along `diag` (tw = the word that holds the last of them): adds to known / refuted
                auto compare = [&]() {
                    const int e = (int)((diag + 15) & 15);  // index of my last base in my word (p0 is a multiple of 16: the same for every lane)
                    // lane 0's left word: the carry, or behind a new seed a load (wave-uniform choice; only lane 0's copy is used)
                    const uint2 tw0 = carry_ok ? make_uint2(c_twx, c_twy) : text.word(diag, (sp << 10) - 16);
                    uint2 twl;
                    twl.x = flx_from_left(tw.x, tw0.x);
                    twl.y = flx_from_left(tw.y, tw0.y);
                    const uint32_t tsl = flx_from_left(ts, carry_ok ? c_ts : 0u);  // (not worth a load: lane 0 behind a new seed refutes its own window only, below)
                    const uint32_t t_own = __builtin_amdgcn_alignbit(twl.x, tw.x, 2 * (15 - e));
                    const uint32_t b_own = (((twl.y & 0xffffu) >> (e + 1)) | (tw.y << (15 - e))) & 0xffffu;  // bit j: my base j is the first of a piece
                    const uint32_t u_own = (((twl.y >> 16) >> (e + 1)) | ((tw.y >> 16) << (15 - e))) & 0xffffu;  // bit j: a unique 13-mer starts at my base j
                    const uint32_t s_own = ((tsl >> (e + 1)) | (ts << (15 - e))) & 0xffffu;  // bit j: the text's 16 bases from my base j on are S1
                    const uint32_t mml = mismatch16(lo ^ t_own);  // bit j: my base j differs from the text
                    const uint32_t mb0 = carry_ok ? c_mb : 0xffffffffu, us0 = carry_ok ? c_us : 0u;
                    const uint32_t mmh = flx_from_left(mml, mb0 & 0xffffu), bh = flx_from_left(b_own, mb0 >> 16);
                    const uint32_t uh = flx_from_left(u_own, us0 & 0xffffu), sh = flx_from_left(s_own, us0 >> 16);
                    const uint32_t z = ~(mmh | (mml << 16));  // bit i: base i of the window [p0 - 16, p0 + 16) matches
                    uint32_t rf = text_verdict(z, bh | (b_own << 16), uh | (u_own << 16), sh | (s_own << 16), valid16, true, known, text12);
                    // (lane 0 behind a new seed knows nothing about the 16 bases in front of it — taken for mismatches above, which is
                    // safe for `known` and would be wrong here: only the window made of its own 16 bases can be refuted)
                    if (lane == 0 && !carry_ok) rf &= 0x8000u;
                    refuted |= rf;
                    c_us = __builtin_amdgcn_readlane(u_own | (s_own << 16), 63);
                    c_ts = __builtin_amdgcn_readlane(ts, 63);
                    c_mb = __builtin_amdgcn_readlane(mml | (b_own << 16), 63);
                    c_twx = __builtin_amdgcn_readlane(tw.x, 63);
                    c_twy = __builtin_amdgcn_readlane(tw.y, 63);
                    carry_ok = true;
                };
                // The carried diagonal is tested for nothing.  Then, while at least three lanes behind the last lane with a known
                // member hold 16-mers nothing is known about (junk, an indel, the end of a piece of the text, the wrong copy of a
                // repeat), two of them look their own 16 bases up in the seed table — eight lanes spread over the span when nothing
                // is known at all; a seed on another diagonal is compared in turn, what it confirms adds to what is known.
                const unsigned long long whole = __ballot((valid16 >> 15) != 0);  // lanes that hold a whole 16-mer of the read
                bool again = have_diag;
                for (int seeds_left = FLX_LOCUS_SEEDS;;) {
                    if (again) compare();
                    const unsigned long long kn = __ballot(known != 0);
                    const unsigned long long tail = kn ? whole & ~((2ull << (63 - __clzll(kn))) - 1ull) : whole;
                    if (seeds_left-- == 0 || __popcll(tail) < FLX_LOCUS_TAIL) break;
                    bool tries;
                    if (kn) {
                        const unsigned long long t1 = tail & (tail - 1), t2 = t1 & (t1 - 1);  // without its first lane / first two lanes
                        tries = lane == __ffsll(t1) - 1 || lane == __ffsll(t2) - 1;
                    } else {
                        tries = (lane & 7) == 3 && ((whole >> lane) & 1ull);
                    }
                    uint32_t tpos = kLocusEmpty;
                    if (tries) tpos = text.seed(lo);
                    const unsigned long long found = __ballot(tpos != kLocusEmpty);
                    if (!found) break;
                    const int src = __ffsll(found) - 1;
                    const long long nd = (long long)__builtin_amdgcn_readlane(tpos, src) - (long long)((sp << 10) + src * 16);
                    if (have_diag && nd == diag) break;  // the same locus: what is missing are mismatches, not the diagonal
                    diag = nd;
                    have_diag = true;
                    carry_ok = false;
                    tw = text.word(diag, sp << 10);
                    ts = text.safe(diag, sp << 10);
                    if (sp + 1 < n_spans) {
                        tw_next = text.word(diag, (sp << 10) + 1024);
                        ts_next = text.safe(diag, (sp << 10) + 1024);
                    }
                    again = true;
                }
            }

            // ---- exact membership (exact_pair_probe): the known members enter the search as confirmed hits ----
            uint32_t hits = known, probed = known;

            // ---- far first (clean stretches): where most lanes of the previous span had their own last 16-mer AND their left
            // neighbour's confirmed, ask for the last 16-mer of every lane before anything else.  A lane whose own and whose left
            // neighbour's are members is SETTLED: its 16 bases lie in its own last 16-mer, the 15 before them in the neighbour's,
            // so none of its other 16-mers can add coverage and its eight prefilter lines are never fetched.  The request is the
            // one a clean lane needs anyway; it is wasted only on a lane whose last pair holds no candidate. ----
            bool settled = false;
            uint32_t ltop = 0;  // far first: is the left neighbour's last 16-mer a member
            if (far_first) {
                const bool ask15 = (valid16 >> 15) != 0 && ((known | refuted) >> 15) == 0;
                if (__any(ask15)) exact_pair_probe(a, hi, lo, ask15 ? 15 : -1, -1, valid16, hits, probed);
                ltop = flx_from_left(hits >> 15, c_hit15);
                settled = (hits >> 15) && ltop;
            } else if (LOCUS) {
                ltop = flx_from_left(known >> 15, c_hit15);
                settled = (known >> 15) && ltop;
            }
            // LOCUS: the 12-mers ending at [lowest hit - 4, highest hit] need no lookup — those inside a member are present, the
            // others only make candidates between two confirmed members, which are never asked
            uint32_t need12 = 0xffffu;
            if (LOCUS && hits) {
                const int a = __ffs(hits) - 1, b = 31 - __clz(hits);
                const int from = a > 4 ? a - 4 : 0;
                need12 = ~(((2u << b) - 1u) & ~((1u << from) - 1u)) & 0xffffu;
            }
            if (LOCUS) need12 &= ~text12;  // (12-mers that match the text between two mismatches less than 16 apart: present without a lookup)

            // ---- 12-mer prefilter: pair m = positions p0 + 2m, p0 + 2m + 1; x.C.y = the 13 bases ending at p0 + 2m + 1 ----
            uint32_t p12 = 0xffffu;  // (a settled lane: every 12-mer of its last 16-mer is present, the others are not needed)
            if (HAS_PREFILTER && !LOCUS && !settled) {
                uint32_t byte[8], sel[8];
                FLX_GLOBAL_PTR(uint8_t) pre11 = FLX_KARG_PTR(uint8_t, pre11);
#pragma unroll
                for (int m = 0; m < 8; ++m) {
                    const uint32_t a = __builtin_amdgcn_alignbit(hi, lo, 28 - 4 * m);
                    const flx_pre11_slot q = flx_pre11((a >> 2) & 0x3FFFFFu, (a >> 24) & 3u, a & 3u);
                    byte[m] = pre11[q.index];
                    sel[m] = q.even_bit | (q.odd_bit << 8);
                }
                p12 = 0;
#pragma unroll
                for (int m = 0; m < 8; ++m)
                    p12 |= (((byte[m] >> (sel[m] & 0xffu)) & 1u) | (((byte[m] >> (sel[m] >> 8)) & 1u) << 1)) << (2 * m);
            }
            if (HAS_PREFILTER && LOCUS) {
                // In TWO rounds: a 16-mer is out as soon as ONE of its five 12-mers is absent, and what is left to look up holds a
                // mismatch against the text, so it is absent more often than not.  Round 1 fetches the even pairs (positions 0 1,
                // 4 5, 8 9, 12 13) where needed; every 16-mer holds two or three of those positions, so most are out after it.
                // Round 2 fetches an odd pair only if one of the six 16-mers that hold its 12-mers — five of them may be the right
                // neighbour's — is still alive under the assumption that every 12-mer not yet seen is present.  A pair that is
                // skipped keeps that assumption: it only concerns 16-mers that are out anyway.
                // (the reverse complement of the whole 32-base window once: the canonical form of every pair's 11-mer is then one
                // funnel shift, and a byte read for the other strand is looked at bit-reversed — bit 7 - x is bit x, bit 3 - y is bit
                // 4 + y — instead of with two selected bit numbers: kmerset.h, flx_pre11, in 19 instead of 33 instructions per pair)
                const uint64_t r64 = ((uint64_t)rc32(lo) << 32) | rc32(hi);
                auto fetch = [&](uint32_t want, int parity) -> uint32_t {  // actual bits of the pairs m = parity, parity + 2, .. that hold a wanted position; 1 elsewhere
                    uint32_t byte[4], got = parity ? 0x3333u : 0xCCCCu;
                    FLX_GLOBAL_PTR(uint8_t) pre11 = FLX_KARG_PTR(uint8_t, pre11);
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const int m = 2 * k + parity;
                        const uint32_t a = __builtin_amdgcn_alignbit(hi, lo, 28 - 4 * m);  // x.C.y, the 13 bases ending at position 2m + 1
                        byte[k] = ((want >> (2 * m)) & 3u) ? pre11[pre11_pair_index(a, (uint32_t)(r64 >> (12 + 4 * m)) & 0x3FFFFFu)] : 0xffu;
                    }
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const int m = 2 * k + parity;
                        const uint32_t a = __builtin_amdgcn_alignbit(hi, lo, 28 - 4 * m);
                        got |= pre11_pair_bits(a, byte[k]) << (2 * m);  // (a pair that was not fetched holds 0xff: both present)
                    }
                    return got;
                };
                const uint32_t want = settled ? 0u : (need12 & valid12);
                {
                    // round 1 as well leaves out the pairs whose 12-mers only lie in 16-mers the text has refuted (U13, S1)
                    uint32_t alive = settled ? 0u : (valid16 & (~refuted | known));
                    const uint32_t right = flx_from_right(alive, 0xffffu);
                    uint32_t dep = alive | (right << 16);
                    dep |= dep >> 1;
                    dep |= dep >> 2;
                    dep |= dep >> 1;
                    const uint32_t w1 = want & 0x3333u & dep;
                    p12 = __any(w1 != 0) ? fetch(w1, 0) : 0xffffu;  // (a span the text settles: nothing is computed for it)
                }
                if (__any((want & 0xCCCCu) != 0)) {
                    const uint32_t v1 = p12 & valid12;
                    const uint32_t l1 = flx_from_left(v1 >> 11, c_p12);
                    const uint32_t m1 = (l1 >> 1) | (v1 << 4);
                    uint32_t alive = m1 & (m1 >> 1) & (m1 >> 2) & (m1 >> 3) & (m1 >> 4) & valid16 & ~refuted;
                    if (settled) alive = 0;  // (a settled lane asks nothing; its neighbours' 16-mers that reach into it count below)
                    const uint32_t right = flx_from_right(alive, 0xffffu);  // (lane 63: the next span's first lane is not known yet)
                    uint32_t dep = alive | (right << 16);
                    dep |= dep >> 1;
                    dep |= dep >> 2;
                    dep |= dep >> 1;  // bit q: one of the 16-mers ending at q .. q + 4 (those that hold the 12-mer ending at q) is alive
                    const uint32_t w2 = want & 0xCCCCu & dep;
                    if (__any(w2 != 0)) p12 &= fetch(w2, 1);
                }
            }
            p12 &= valid12;
            uint32_t p12_left = flx_from_left(p12 >> 11, c_p12);  // the left lane's 12-mers ending at its positions 11..15 = mine at -5..-1
            if (!HAS_PREFILTER) p12_left = 0x1fu;
            const uint32_t m12 = (p12_left >> 1) | (p12 << 4);  // bit i: the 12-mer ending at p0 - 4 + i
            uint32_t cand = m12 & (m12 >> 1) & (m12 >> 2) & (m12 >> 3) & (m12 >> 4) & valid16;  // all five 12-mers present
            if (LOCUS) cand &= ~refuted | known;  // (a member known on one diagonal cannot be refuted on another — its 13-mers then occur twice in the text — but nothing is lost by saying so)
            if (settled) cand = hits;  // nothing open: the confirmed members are all this lane contributes
            const uint32_t lcand = flx_from_left(cand >> 15, c_cand15);
            hits &= cand;  // (a member is always a candidate)
            probed |= ~cand & 0xffffu;

            // the search for the outermost members, one step (next_asks) and one request per side at a time
            uint32_t lhit;
            int top, bot;
            if (far_first) {
                lhit = ltop & lcand;  // already exact
            } else {
                // first step on a BET: a candidate at the left neighbour's last position is taken for a member (it is the top of
                // that lane's search, so its answer arrives with this round's), corrected right after
                const bool need = next_asks(cand, hits, probed, lcand, top, bot);
                if (__any(need)) exact_pair_probe(a, hi, lo, top, bot, cand, hits, probed);
                lhit = flx_from_left(hits >> 15, c_hit15) & lcand;
            }
            for (;;) {
                const bool need = next_asks(cand, hits, probed, lhit, top, bot);
                if (!__any(need)) break;
                exact_pair_probe(a, hi, lo, top, bot, cand, hits, probed);
            }

            // far first for the next span?  Per lane the skipped prefilter lines are worth 8 x 3.8 ps, a wasted request 18 ps
            // (tools/tabench): worth it from about half the lanes settled.
            if (LOCUS) {  // lanes the text settles anyway do not count: they ask nothing either way
                const uint32_t lknown = flx_from_left(known >> 15, c_known15);
                far_first = __popcll(__ballot((hits >> 15) && lhit && !((known >> 15) && lknown))) >= FLX_FARFIRST_LANES_LOCUS;
                c_known15 = __builtin_amdgcn_readlane(known >> 15, 63);
            } else {
                far_first = __popcll(__ballot((hits >> 15) && lhit)) >= FLX_FARFIRST_LANES;
            }

            // ---- coverage of the previous span (its lane 63 needed my lane 0's hits), then carry ----
            if (sp > 0) emit_piece<SEGMENTS>(rd, sp - 1, lane, prev_hits, flx_from_right(prev_hits, __builtin_amdgcn_readfirstlane(hits)), tally);
            prev_hits = hits;
            c_lo = __builtin_amdgcn_readlane(lo, 63);
            c_p12 = __builtin_amdgcn_readlane(p12 >> 11, 63);
            c_cand15 = __builtin_amdgcn_readlane(cand >> 15, 63);
            c_hit15 = __builtin_amdgcn_readlane(hits >> 15, 63);
            raw = raw_next;
            if (LOCUS) {
                tw = tw_next;
                ts = ts_next;
            }
        }
        if (n_spans > 0) emit_piece<SEGMENTS>(rd, n_spans - 1, lane, prev_hits, flx_from_right(prev_hits, 0u), tally);
        wave_reduce_and_store<SEGMENTS>(a, rd, lane, tally);
    }
}

}  // namespace

template <bool SEGMENTS>
static void launch_cover_w(const CoverArgs &ca, bool prefilter, bool locus, unsigned grid, hipStream_t st) {
    if (prefilter && locus)
        hipLaunchKernelGGL((k_kmer_cover_w<true, true, SEGMENTS>), dim3(grid), dim3(FLX_COVER_THREADS), 0, st, ca);
    else if (prefilter)
        hipLaunchKernelGGL((k_kmer_cover_w<true, false, SEGMENTS>), dim3(grid), dim3(FLX_COVER_THREADS), 0, st, ca);
    else if (locus)
        hipLaunchKernelGGL((k_kmer_cover_w<false, true, SEGMENTS>), dim3(grid), dim3(FLX_COVER_THREADS), 0, st, ca);
    else
        hipLaunchKernelGGL((k_kmer_cover_w<false, false, SEGMENTS>), dim3(grid), dim3(FLX_COVER_THREADS), 0, st, ca);
}

// FLX_KMER_COVER: "v2" = round 2's workgroup-per-read kernel, "w" = the wave-level kernel of rounds 3-5 for every set (second
// and third implementation; default: k_kmer_cover_q, cover_queue.hip, for a set with a text, k_kmer_cover_w for one without),
// "q2" = k_kmer_cover_q with EVERY read in its second launch (a diagonal per lane: tests)
static bool cover_env_is(const char *value) {
    const char *env = getenv("FLX_KMER_COVER");
    return env && strcmp(env, value) == 0;
}

bool flx_kmer_cover_is_v2(const flx_kmerset *set) {
    return cover_env_is("v2") || !flx_kmerset_exact15(set);  // (no pair table: finalize found no room for it)
}

int flx_kmer_cover_stage(flx_ctx *ctx, const flx_kmerset *set, const uint8_t *d_plane, const uint64_t *d_offsets, const int32_t *d_lengths, const uint32_t *d_order,
                         uint64_t n_reads, uint32_t *d_cov, const uint64_t *d_covoff, int32_t *d_count, int32_t *d_first, int32_t *d_last, uint8_t *d_redo,
                         CoverLong &cvl, CoverLongCounts *d_long_counts, void *long_work, size_t long_work_bytes) {
    hipStream_t st = ctx->stream;
    flx_time_scope tc(ctx, "flx_score_kmer_cover");
    ctx->last_kmer_locus = false;
    ctx->last_kmer_cover = "v2";
    if (flx_kmer_cover_is_v2(set)) {
        const unsigned grid = (unsigned)std::min<uint64_t>(n_reads, 1u << 20);
        hipLaunchKernelGGL(k_kmer_cover<256>, dim3(grid), dim3(256), 0, st, d_plane, d_offsets, d_lengths, d_order, n_reads, flx_kmerset_bitmap(set),
                           flx_kmerset_prefilter(set), d_cov, d_covoff, d_count, d_first, d_last);
        hipLaunchKernelGGL(k_kmer_cover<64>, dim3(grid), dim3(64), 0, st, d_plane, d_offsets, d_lengths, d_order, n_reads, flx_kmerset_bitmap(set),
                           flx_kmerset_prefilter(set), d_cov, d_covoff, d_count, d_first, d_last);
        return FLX_OK;
    }
    const bool wave_cover = cover_env_is("w");
    const bool second_only = cover_env_is("q2");  // every read through the kernel with a diagonal per lane (tests)
    const unsigned wgrid = (unsigned)std::min<uint64_t>((n_reads + FLX_COVER_THREADS / 64 - 1) / (FLX_COVER_THREADS / 64), 1u << 22);
    const char *locus_env = getenv("FLX_KMER_LOCUS");  // "0": without the assembly text (the round-3 kernel; tests, A/B)
    const flx_locus *lp = (locus_env && locus_env[0] == '0') ? nullptr : flx_kmerset_locus(set);
    flx_locus none;
    memset(&none, 0, sizeof none);
    ctx->last_kmer_locus = lp != nullptr;
    const uint8_t *pre11 = flx_kmerset_pre11(set);
    const bool queue = lp && !wave_cover;
    CoverArgs ca = {d_plane, d_offsets, d_lengths, d_order, n_reads, flx_kmerset_exact15(set), pre11, lp ? *lp : none, d_cov, d_covoff, d_count, d_first, d_last, d_redo,
                    cvl.on ? (uint32_t)cvl.thr : kCoverNoLong, nullptr};
    ctx->last_kmer_cover = queue ? (second_only ? "q2" : "q") : "w";
    // one launch of the form this call runs: on the batch, then (segments) on the segment table of its long reads
    auto launch_cover = [&](const CoverArgs &args, unsigned g, bool segments) -> int {
        if (queue) return flx_cover_queue_launch(ctx, args, pre11 != nullptr, g, second_only, segments);
        if (segments) launch_cover_w<true>(args, pre11 != nullptr, lp != nullptr, g, st);
        else launch_cover_w<false>(args, pre11 != nullptr, lp != nullptr, g, st);
        return FLX_OK;
    };
    if (queue) {  // (the batch's marks: flx_last_kmer_handed_over does not count the segments')
        ctx->last_kmer_redo = d_redo;
        ctx->last_kmer_redo_n = n_reads;
    }
    FLX_CHECK(launch_cover(ca, wgrid, false));
    tc.end();
    if (cvl.n.n_segs) {
        // The long reads, one wave per segment.  A bracket of its own behind the batch's (brackets of one stage do not nest):
        // flx_timing_get("flx_score_kmer_cover") still sums the whole stage's device time
        flx_time_scope tl(ctx, "flx_score_kmer_cover.long");
        CoverArgs sa;
        FLX_CHECK(flx_cover_long_table(ctx, cvl, ca, d_long_counts, long_work, long_work_bytes, &sa));
        const unsigned sgrid = (unsigned)std::min<uint64_t>((sa.n_reads + FLX_COVER_THREADS / 64 - 1) / (FLX_COVER_THREADS / 64), 1u << 22);
        FLX_CHECK(launch_cover(sa, sgrid, true));
        FLX_CHECK(flx_cover_long_reduce(ctx, cvl, ca, long_work));
    }
    return FLX_OK;
}
