// score_kmer.hip — k-mer mode per-read scoring on gfx950: the window folds over the coverage bits, and the call that runs both stages.
//
// Replaces the k-mer branch of the reference's Read::Read: first/last covered base (src/read.cpp:75-84), bad ranges /
// trim / split -> child ranges (86-130) and the scoring of every child read (131-141), plus the shared
// mean / window / cut-off code (208-236, 64-73).  The lookups that turn the seq plane into the coverage bit plane (43-58) are the
// coverage stage's: cover_common.h (flx_kmer_cover_stage), cover_wave.hip, cover_queue.hip, cover_long.hip.
//
//   k_kmer_fold   (read-serial)  one lane per read walks its coverage bits and replays get_window_quality
//                 bit-exactly (w -= q[i]/ws; w += q[j]/ws with q/ws in {0, fl(1/ws)}: the drift is real,
//                 SURVEY §8c test_trim_3 = 0x1.5ffffffffffffp+6), and — under --trim/--split — finds the bad
//                 zero-runs, the child ranges, and runs the same recurrence for every child on the fly.
//                 Children never have grandchildren (their coverage is a slice of the parent's),
//                 so a child's mean/window/cut-offs come from the parent's bits without new lookups.
#include "flx_internal.h"
#include "kmerset.h"
#include "cover_common.h"
#include "rank_internal.h"
#include "score_kmer_common.h"

namespace {

// ---------------------------------------------------------------------------------------------------
// serial fold over the coverage bits
// ---------------------------------------------------------------------------------------------------
#ifndef FLX_FOLD_FMA
#define FLX_FOLD_FMA 1
#endif
// (the grid table, the folds' arguments and the shared result code: fold_grid_tab.h, score_kmer_common.h)
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
#ifndef FLX_FOLD_WALK_COPIES
#define FLX_FOLD_WALK_COPIES 1  // copies of the integer-grid fold's walk table in LDS (a power of two; 1, 8, 16 measured: no difference — the gathers are not what bounds the kernel)
#endif
#ifdef FLX_FOLD_WAVES_PER_EU  // (A/B builds: the register budget of the fold kernels)
#define FLX_FOLD_OCC __attribute__((amdgpu_waves_per_eu(FLX_FOLD_WAVES_PER_EU)))
#else
#define FLX_FOLD_OCC
#endif
template <int MODE, bool RING, bool GRID = false>
__global__ void __launch_bounds__(256) FLX_FOLD_OCC k_kmer_fold(const FoldArgs a) {
    const uint64_t slot = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool live = slot < (MODE == 6 ? a.n_children : a.n_reads);
    uint32_t rid = 0;  // MODE 6: the child's index
    int L = 0;
    const uint32_t *row = a.cov;
    int row_words_left = 0;       // MODE 6: words of the parent's row from `row` on
    uint32_t bit_off = 0;         // MODE 6: the child starts at bit `bit_off` (0..127) of row[0]
    if (live && MODE != 6) {
        rid = a.order ? a.order[slot] : (uint32_t)slot;
        L = a.lengths[rid];
        row = a.cov + (a.cov_off[rid] >> 2);
    }
    if (live && MODE == 6) {
        rid = a.child_order[slot];
        const uint32_t parent = a.child_parent[rid];
        const int start = a.child_ranges[2 * (size_t)rid], end = a.child_ranges[2 * (size_t)rid + 1];
        L = end - start;
        const int base_word = (start >> 7) << 2;  // 16-byte aligned piece of the row the child starts in
        row = a.cov + (a.cov_off[parent] >> 2) + base_word;
        row_words_left = ((a.lengths[parent] + 31) >> 5) - base_word;
        bit_off = (uint32_t)(start - 32 * base_word);
    }
    if ((MODE == 0 || MODE == 3 || MODE == 5 || MODE == 6) && a.long_min > 0 && L >= a.long_min) {
        // a long read or child: the cooperative path's (score_kmer_long.hip) — this lane folds nothing and writes nothing
        live = false;
        L = 0;
    }
    int Lmax = L;
    for (int o = 32; o > 0; o >>= 1) Lmax = max(Lmax, __shfl_xor(Lmax, o, 64));
    const int ws = a.ws;
    const double delta = a.delta;

    Win P = {0, 0.0, 0.0};
    // child machinery
    Win C = {0, 0.0, 0.0};
    Win S = {0, 0.0, 0.0};  // snapshot of C at the start of the current zero run
    int cs = 0;             // start of the current child candidate
    int zs = -1;            // start of the current zero run (-1: none)
    bool any_bad = false;
    uint32_t nchild = 0;
    const uint64_t cbase = ((MODE == 2 || MODE == 4 || MODE == 5) && live) ? a.child_offsets[rid] : 0;
    const bool split_set = a.p.split_set != 0;
    const bool trim = a.p.trim != 0;
    const int split = a.p.split;

    auto emit_child = [&](int start, int end, const Win &st) {
        if (end <= start) return;
        if (MODE == 5) {
            const uint64_t at = cbase + nchild;
            a.child_ranges[2 * at] = start;
            a.child_ranges[2 * at + 1] = end;
            a.child_parent[at] = rid;
        }
        if (MODE == 3 && a.inline_ranges && nchild < (uint32_t)kInlineChildren) {
            int32_t *slot = a.inline_ranges + ((size_t)rid * kInlineChildren + nchild) * 2;
            slot[0] = start;
            slot[1] = end;
        }
        if (MODE == 2 || MODE == 4) {
            const int len = end - start;
            const double mean = 100.0 * (double)st.cnt / (double)len;
            const double window = window_result(a, len, st.cnt, st.mn);
            const uint64_t at = cbase + nchild;
            a.child_ranges[2 * at] = start;
            a.child_ranges[2 * at + 1] = end;
            a.child_mean_q[at] = mean;
            a.child_window_q[at] = window;
            a.child_passed[at] = cutoffs(a.p, len, mean, window);
        }
        ++nchild;
    };

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
    const int n_words = MODE == 6 ? row_words_left : (L + 31) >> 5;  // words of the row that exist behind `row`
    const int o5 = (int)(bit_off >> 5);                                // MODE 6: the child's word k = row words k + o5, k + o5 + 1 ...
    const unsigned o = bit_off & 31u;                                  // ... shifted right by o bits
    auto ldq = [&](int b) -> uint4 {
        return (b * 4 < n_words) ? *reinterpret_cast<const uint4 *>(row + 4 * (size_t)b) : make_uint4(0u, 0u, 0u, 0u);
    };
    struct WStream { uint4 cur, nxt; int blk; };
    auto advance = [&](WStream &st, int b) {  // streams only move forward, one block at a time
        if (b != st.blk) {
            st.cur = st.nxt;
            st.blk = b;
            st.nxt = ldq(b + 1);
        }
    };
    auto word = [&](const WStream &st, int wi) -> uint32_t {  // wi inside block st.blk or st.blk + 1
        // (selects, no reference to one of the two blocks: a reference makes the compiler keep the stream in scratch memory)
        const bool cur = (wi >> 2) == st.blk;
        const int c = wi & 3;
        const uint32_t x = cur ? st.cur.x : st.nxt.x, y = cur ? st.cur.y : st.nxt.y, z = cur ? st.cur.z : st.nxt.z, w = cur ? st.cur.w : st.nxt.w;
        const uint32_t v = c == 0 ? x : c == 1 ? y : c == 2 ? z : w;
        return wi < n_words ? v : 0u;  // the padding of the last block is not coverage
    };
    WStream lead = {make_uint4(0u, 0u, 0u, 0u), make_uint4(0u, 0u, 0u, 0u), 0};
    if (!RING) lead = {ldq(0), ldq(1), 0};
    WStream trail = lead;
    extern __shared__ uint32_t fold_ring[];
    const int R = a.ring_words;  // power of two >= 16 + ceil(ws / 32) + 2
    // GRID: in front of the rings the table of the +-1 walk of four positions, indexed by (new nibble << 4 | old nibble): two dwords,
    // {lowest prefix, -(highest prefix)} and {total, -total} as pairs of 16-bit integers (packed adds and minima carry both at once)
    // ... and behind it the grid table itself (GridTab: d* and the lower bound per binade, 4 dwords per entry): a regime begins in
    // the middle of the steady state, and a load from the kernel's arguments there costs the whole wave a trip to memory
    // (kWalkCopies copies of the walk table, entry idx of copy c at (idx * copies + c): a lane reads copy lane % copies, so that
    // lanes with different nibble pairs rarely meet in one bank — with one copy the 64 lanes of a gather share 32 bank pairs)
    constexpr int kWalkCopies = FLX_FOLD_WALK_COPIES;
    constexpr int kGridTabAt = 512 * kWalkCopies;  // dword index of the grid table
    constexpr int kWalkWords = GRID ? kGridTabAt + 8 * 32 : 0;
    if (GRID) {
        for (int i = threadIdx.x; i < GridTab::kMax; i += blockDim.x) {
            fold_ring[kGridTabAt + 8 * i + 0] = (uint32_t)__double2loint(a.gt.dstar[i]);
            fold_ring[kGridTabAt + 8 * i + 1] = (uint32_t)__double2hiint(a.gt.dstar[i]);
            fold_ring[kGridTabAt + 8 * i + 2] = (uint32_t)__double2loint(a.gt.lv[i]);
            fold_ring[kGridTabAt + 8 * i + 3] = (uint32_t)__double2hiint(a.gt.lv[i]);
            fold_ring[kGridTabAt + 8 * i + 4] = (uint32_t)a.gt.top[i];
        }
        for (int idx = threadIdx.x; idx < 256; idx += blockDim.x) {
            int t = 0, mp = 0, xp = 0;
            for (int i = 0; i < 4; ++i) {
                t += ((idx >> (4 + i)) & 1) - ((idx >> i) & 1);
                mp = min(mp, t);
                xp = max(xp, t);
            }
            for (int c = 0; c < kWalkCopies; ++c) {
                fold_ring[2 * (idx * kWalkCopies + c)] = ((uint32_t)mp & 0xffffu) | ((uint32_t)(-xp) << 16);
                fold_ring[2 * (idx * kWalkCopies + c) + 1] = ((uint32_t)t & 0xffffu) | ((uint32_t)(-t) << 16);
            }
        }
        __syncthreads();
    }
    uint32_t *ring = fold_ring + kWalkWords + (size_t)(threadIdx.x >> 6) * (size_t)R * 64 + (threadIdx.x & 63);
    uint4 nq[4];       // the block after the newest one in the ring
    int have_blk = -1;  // newest block in the ring (wave-uniform: every lane is at the same position)
    if (RING) {
#pragma unroll
        for (int q = 0; q < 4; ++q) nq[q] = ldq(q);
    }
    auto ring_fill = [&](int wi) {  // word wi (and everything up to the end of its block) into the ring; wi only moves forward
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
    };
    auto ring_word = [&](int wi) -> uint32_t { return wi < n_words ? ring[(wi & (R - 1)) * 64] : 0u; };
    // MODE 6: bit p of the child is bit p + bit_off of the row, so 32 child positions from position p on are row words
    // (p + bit_off) / 32 and the next one, funnel-shifted by (p + bit_off) mod 32
    auto lead_bits = [&](int p) -> uint32_t {  // p a multiple of 32, moving forward
        const int w = (p >> 5) + o5;
        uint32_t lo, hi;
        if (RING) { ring_fill(w + 1); lo = ring_word(w); hi = ring_word(w + 1); }
        else { advance(lead, w >> 2); lo = word(lead, w); hi = word(lead, w + 1); }
        return __builtin_amdgcn_alignbit(hi, lo, o);
    };
    auto trail_bits = [&](int p) -> uint32_t {  // any p >= 0 behind the leading edge, moving forward
        const int t = p + (int)bit_off, w = t >> 5;
        uint32_t lo, hi;
        if (RING) { lo = ring_word(w); hi = ring_word(w + 1); }
        else { advance(trail, w >> 2); lo = word(trail, w); hi = word(trail, w + 1); }
        return __builtin_amdgcn_alignbit(hi, lo, (unsigned)(t & 31));
    };
    auto lead_word = [&](int wi) -> uint32_t {  // the word holding the leading edge
        if (MODE == 6) return lead_bits(wi << 5);
        if (RING) { ring_fill(wi); return ring_word(wi); }
        advance(lead, wi >> 2);
        return word(lead, wi);
    };
    auto trail_word = [&](int wi) -> uint32_t {  // words of the trailing edge: never ahead of the leading one
        if (MODE == 6) return trail_bits(wi << 5);
        if (RING) return ring_word(wi);
        advance(trail, wi >> 2);
        return word(trail, wi);
    };
    uint32_t lead_w = 0, trail_w = 0;
    int Lmin = live ? L : 0x7fffffff;
    for (int o = 32; o > 0; o >>= 1) Lmin = min(Lmin, __shfl_xor(Lmin, o, 64));
    const unsigned int d_lo = (unsigned int)(__double_as_longlong(delta) & 0xffffffffll);
    const unsigned int d_hi = (unsigned int)(__double_as_longlong(delta) >> 32);
    // GRID: the regime of this lane's parent window (w = g_wb + g_c * g_ds while it holds; lowest c so far in g_cmin)
    double g_wb = 0.0, g_ds = 0.0;
    int g_c = 0, g_cmin = 0, g_lo = 0x7fffffff, g_hi = (int)0x80000000;
    bool grid_on = false;  // wave-uniform: the steady state has begun (and not ended)
    auto grid_flush = [&]() {  // the regime's state as the recurrence's: exact, every operand is a multiple of the regime's grid
        P.mn = fmin(P.mn, fma((double)g_cmin, g_ds, g_wb));
        P.w = fma((double)g_c, g_ds, g_wb);
    };
    auto grid_begin = [&]() {  // a regime from P.w on (tools/sim_fold_grid.cpp: begin_regime — the same arithmetic)
        g_wb = P.w;
        g_ds = 0.0;
        g_c = 0;
        g_cmin = 0;
        g_lo = 0x7fffffff;
        g_hi = (int)0x80000000;
        const int eb = (__double2hiint(P.w) >> 20) & 0x7ff;
        const int idx = eb - a.gt.e0;
        if (P.w > 0.0 && idx >= 0 && idx < a.gt.n) {
            const uint4 e = *reinterpret_cast<const uint4 *>(fold_ring + kGridTabAt + 8 * idx);
            const double ds = __hiloint2double((int)e.y, (int)e.x), lv = __hiloint2double((int)e.w, (int)e.z);
            if (ds > 0.0) {
                // The top: w must not reach a binade on whose grid w_b does NOT lie (its low bits would be rounded away there).  w_b
                // lies on the grid of binade eb + z, z = the trailing zero bits of its mantissa — a window that has once been full
                // (w = 1.0) stays on the grid of [1, 2) whatever is subtracted, d* is a multiple of it — up to the top of the group.
                const uint32_t m_lo = (uint32_t)__double2loint(P.w), m_hi = ((uint32_t)__double2hiint(P.w) & 0xfffffu) | 0x100000u;
                const int z = m_lo ? __ffs((int)m_lo) - 1 : 32 + (__ffs((int)m_hi) - 1);
                const int gb = min(eb + z, (int)fold_ring[kGridTabAt + 8 * idx + 4]);
                const double uv = __hiloint2double((gb + 1) << 20, 0);
                // smallest c with w + c d* > lv: the estimate's floor is the answer or up to two below it; the values decide
                int k0 = (int)floor((lv - P.w) * a.ws_d);
                if (fma((double)k0, ds, P.w) <= lv) ++k0;
                if (fma((double)k0, ds, P.w) <= lv) ++k0;
                // largest c with w + c d* < uv
                int k1 = (int)ceil((uv - P.w) * a.ws_d);
                if (fma((double)k1, ds, P.w) >= uv) --k1;
                if (fma((double)k1, ds, P.w) >= uv) --k1;
                g_ds = ds;
                g_lo = k0;
                g_hi = k1;
            }
        }
    };
    for (int j0 = 0; j0 < Lmax; j0 += 32) {
      lead_w = lead_word(j0 >> 5);
      if (MODE == 4) {
          // ---- children only: events per word, then 32 predicated positions ----
          int ev_end = -1, ev_zs = 0, snap = -1;
          if (j0 < L) {
              const int v = min(32, L - j0);
              const uint32_t w = v < 32 ? (lead_w & ((1u << v) - 1u)) : lead_w;
              if (j0 == 0 && !(w & 1u)) zs = 0;  // S is still the initial (empty) state
              if (w != 0) {
                  if (zs >= 0) {
                      const int f = __ffs(w) - 1;
                      const bool bad = (split_set && j0 + f - zs >= split) || (trim && zs == 0);
                      if (bad) { ev_end = f; ev_zs = zs; }
                      zs = -1;
                  }
                  const int top = 32 - __clz(w);
                  if (top < v) { zs = j0 + top; snap = top; }
              } else if (zs < 0) {
                  zs = j0;
                  snap = 0;
              }
          }
          // trailing window of the 32 positions (positions before the read count as uncovered; they are never used,
          // a child's trailing edge lies inside the child)
          const int tj0 = j0 - ws;
          uint32_t tw = 0;
          if (tj0 > -32) {
              const int twi = tj0 >> 5, sh = tj0 & 31;  // twi == -1 for the word that straddles position 0
              const uint32_t lo = twi >= 0 ? trail_word(twi) : 0u;
              tw = sh ? __builtin_amdgcn_alignbit(trail_word(twi + 1), lo, (unsigned)sh) : lo;
          }
#pragma unroll
          for (int i = 0; i < 32; ++i) {
              const int j = j0 + i;
              if (i == ev_end) {  // a bad range ended here: the child [cs, ev_zs) is complete, a new one starts at j
                  any_bad = true;
                  emit_child(cs, ev_zs, S);
                  cs = j;
                  C.cnt = 0;
                  C.w = 0.0;
                  C.mn = 0.0;
              }
              if (i == snap) {  // state of the current child at the start of a zero run that may turn out bad
                  S.cnt = C.cnt;
                  S.mn = C.mn;
              }
              const bool act = j < L;
              const int k = j - cs;
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
          continue;
      }
      if ((MODE == 3 || MODE == 5) && j0 < L) {
          const int v = min(32, L - j0);  // valid bits of this word
          const uint32_t w = v < 32 ? (lead_w & ((1u << v) - 1u)) : lead_w;
          if (j0 == 0 && !(w & 1u)) zs = 0;  // the read starts inside a zero run
          if (w != 0) {
              if (zs >= 0) {  // the run [zs, j) that reached this word ends at its first covered base
                  const int j = j0 + __ffs(w) - 1;
                  const bool bad = (split_set && j - zs >= split) || (trim && zs == 0);
                  if (bad) {
                      any_bad = true;
                      emit_child(cs, zs, S);  // (counts it; MODE 5 also writes its range)
                      cs = j;
                  }
                  zs = -1;
              }
              const int top = 32 - __clz(w);  // one past the last covered base of the word
              if (top < v) zs = j0 + top;     // the word ends inside a new zero run
          } else if (zs < 0) {
              zs = j0;
          }
      }
      if (MODE == 5) continue;
      if ((MODE == 0 || MODE == 3 || MODE == 6) && j0 + 32 <= ws - 1 && j0 + 32 <= Lmin) {
          // ---- the head, a word at a time: every position of the word lies in front of the first full window (j < ws - 1) and inside
          // every read of the wave — the recurrence has not begun, only the covered bases are counted (src/read.cpp:221-225).  (The
          // per-bit loop below spent ~20 instructions on each of these positions: a fifth of a 10 kbp read's fold once the steady state
          // ran on the integer grid.)
          P.cnt += __popc(lead_w);
          continue;
      }
      if ((MODE == 0 || MODE == 3 || MODE == 6) && j0 >= ws && j0 + 32 <= Lmin) {
          // ---- steady state, one window per lane: 32 positions, every lane active, no per-bit control flow ----
          uint32_t tw;
          if (MODE == 6) {
              tw = trail_bits(j0 - ws);
          } else {
              const int tj0 = j0 - ws, sh = tj0 & 31, twi = tj0 >> 5;
              const uint32_t t0 = trail_word(twi);
              tw = sh ? __builtin_amdgcn_alignbit(trail_word(twi + 1), t0, (unsigned)sh) : t0;
          }
          P.cnt += __popc(lead_w);
          if (GRID) {
              if (!grid_on) {
                  grid_begin();
                  grid_on = true;
              }
              typedef short s16x2 __attribute__((ext_vector_type(2)));
              // the (new, old) nibble pairs of the word: byte k of `even` = nibbles 2k, of `odd` = nibbles 2k + 1
              const uint32_t odd = (lead_w & 0xF0F0F0F0u) | ((tw >> 4) & 0x0F0F0F0Fu);
              const uint32_t even = ((lead_w << 4) & 0xF0F0F0F0u) | (tw & 0x0F0F0F0Fu);
              const uint2 *walk = reinterpret_cast<const uint2 *>(fold_ring) + (threadIdx.x & (kWalkCopies - 1));
              s16x2 run = {0, 0}, ext = {0, 0};  // {prefix, -prefix} so far; {lowest prefix, -(highest prefix)}
#pragma unroll
              for (int k = 0; k < 8; ++k) {
                  const uint32_t idx = ((k & 1 ? odd : even) >> (8 * (k >> 1))) & 0xffu;
                  const uint2 e = walk[idx * kWalkCopies];
                  ext = __builtin_elementwise_min(ext, run + __builtin_bit_cast(s16x2, e.x));
                  run = run + __builtin_bit_cast(s16x2, e.y);
              }
              const int mp = ext.x, xp = -(int)ext.y, t = run.x;
              // not a no-op (a word of zeros on both edges changes nothing in any regime) and outside the regime: this lane's word in FP
#ifdef FLX_FOLD_GRID_NOSLOW  // (timing experiment only: wrong results)
              const bool slow = false;
#else
              const bool slow = (lead_w | tw) != 0u && !(g_c + mp >= g_lo && g_c + xp <= g_hi);
#endif
              if (!__any(slow)) {
                  g_cmin = min(g_cmin, g_c + mp);
                  g_c += t;
                  continue;
              }
              if (!slow) {
                  g_cmin = min(g_cmin, g_c + mp);
                  g_c += t;
                  lead_w = tw = 0;  // (32 exact no-ops below)
              } else {
                  grid_flush();
              }
              // (four rounds of eight steps, not 32 unrolled: unrolled, the compiler converts all 64 bits to doubles ahead of the chain
              // and the kernel needs 122 registers, or spills)
#pragma unroll 1
              for (int i0 = 0; i0 < 32; i0 += 8) {
#pragma unroll
                  for (int i = 0; i < 8; ++i) {
                      const double lb = (double)__builtin_amdgcn_ubfe(lead_w, i0 + i, 1);
                      const double tb = (double)__builtin_amdgcn_ubfe(tw, i0 + i, 1);
                      P.w = fma(tb, -delta, P.w);
                      P.w = fma(lb, delta, P.w);
                      P.mn = fmin(P.mn, P.w);
                  }
              }
              if (slow) grid_begin();
              continue;
          }
          if (a.events) {
              // Round-3 review, item 5: only the positions where the two edges DIFFER change w for certain (one exact step each);
              // where both are 0 nothing happens, and where both are 1 the step is fl(fl(w - d) + d), which is w itself unless the
              // subtraction leaves w's binade — checked once per stretch of such positions, with the 32-step loop below as the
              // fallback for a word where it fails.  Lanes diverge (a wave runs as many rounds as its busiest lane has events).
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
              if (!__any(slow)) continue;
              if (!slow) {
                  lead_w = tw = 0;  // (this lane is done with the word: 32 exact no-ops below)
              } else {
                  P.w = w0;
                  P.mn = mn0;
              }
          }
#pragma unroll
          for (int i = 0; i < 32; ++i) {
#if FLX_FOLD_FMA
              // w - q[j-ws]/ws and + q[j]/ws with q in {0.0, 1.0} (src/read.cpp:228-229) as fma(bit, -+delta, w): the product is exact
              // (0 or delta), so the one rounding of the fma is the rounding of the reference's subtraction / addition, and
              // adding a zero product leaves w as it is.  7 VALU instructions per position instead of 9 — the folds are VALU bound.
              const double lb = (double)__builtin_amdgcn_ubfe(lead_w, i, 1);
              const double tb = (double)__builtin_amdgcn_ubfe(tw, i, 1);
              P.w = fma(tb, -delta, P.w);
              P.w = fma(lb, delta, P.w);
#else
              const int ml = __builtin_amdgcn_sbfe((int)lead_w, i, 1);  // 0 or -1
              const int mt = __builtin_amdgcn_sbfe((int)tw, i, 1);
              const double dl = __hiloint2double((int)(d_hi & (unsigned)ml), (int)(d_lo & (unsigned)ml));
              const double dt = __hiloint2double((int)(d_hi & (unsigned)mt), (int)(d_lo & (unsigned)mt));
              P.w -= dt;
              P.w += dl;
#endif
              P.mn = fmin(P.mn, P.w);
          }
          continue;
      }
      if (GRID && grid_on) {  // the steady state is over (the shortest read of the wave ends inside this word): back to the recurrence's own state
          grid_flush();
          grid_on = false;
          g_ds = 0.0;
          g_c = g_cmin = 0;
          g_wb = P.w;
      }
      for (int jj = 0; jj < 32; ++jj) {
        const int j = j0 + jj;
        if (j >= Lmax) break;
        const int tj = j - ws;
        if (tj >= 0 && ((tj & 31) == 0 || jj == 0)) {
            trail_w = trail_word(tj >> 5);
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
            if (MODE == 1 || MODE == 2) {
                // ---- zero runs -> bad ranges -> children (src/read.cpp:89-141) ----
                if (b == 0 && zs < 0) {
                    zs = j;
                    S = C;
                }
                if (b == 1 && zs >= 0) {  // the run [zs, j) has ended
                    const bool bad = (split_set && j - zs >= split) || (trim && zs == 0);
                    if (bad) {
                        any_bad = true;
                        emit_child(cs, zs, S);
                        cs = j;
                        C.cnt = 0;
                        C.w = 0.0;
                        C.mn = 0.0;
                    }
                    zs = -1;
                }
                const int k = j - cs;  // position inside the current child
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
    if (GRID && grid_on) grid_flush();
    if (!live) return;

    if (MODE == 6) {  // the child's own scores (src/read.cpp:131-137 -> the Read constructor's folds on the child's slice)
        const double mean = 100.0 * (double)P.cnt / (double)L;
        const double window = window_result(a, L, P.cnt, P.mn);
        a.child_mean_q[rid] = mean;
        a.child_window_q[rid] = window;
        a.child_passed[rid] = cutoffs(a.p, L, mean, window);
        return;
    }
    if (MODE != 0) {
        int end = L;
        if (zs >= 0) {  // the read ends inside a zero run [zs, L)
            const bool bad = (split_set && L - zs >= split) || (trim && zs > 0);
            if (bad) {
                any_bad = true;
                end = zs;
                C = S;
            }
        }
        if (any_bad) emit_child(cs, end, C);
        else nchild = 0;
    }
    if (MODE == 1 || MODE == 3) a.n_child[rid] = nchild;
    if (MODE != 2 && MODE != 4 && MODE != 5) {
        const double mean = 100.0 * (double)a.count[rid] / (double)L;  // exact: the qualities are 0.0 / 1.0
        const double window = window_result(a, L, P.cnt, P.mn);
        a.mean_q[rid] = mean;
        a.window_q[rid] = window;
        a.passed[rid] = cutoffs(a.p, L, mean, window);
    }
}

// (long_min > 0: also counts the batch's long reads and their 32-position steps for the cooperative path, score_kmer_long.hip;
// cover_min > 0: the reads the coverage stage covers in segments, and their segments — cover_long.hip)
__global__ void k_cov_row_bytes(uint64_t n, const int32_t *lengths, int64_t *row_bytes, int long_min, int ws, KmerLongCounts *long_reads,
                                int cover_min, int seg_bases, CoverLongCounts *cover_long) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int L = lengths[i];
    row_bytes[i] = (int64_t)((((uint64_t)L + 7) / 8 + 15) & ~15ull);
    if (long_min > 0 && L >= long_min) {
        atomicAdd(&long_reads->n, 1ull);
        atomicAdd(&long_reads->words, flx_kmer_long_words(L, ws));
    }
    if (cover_min > 0 && L >= cover_min) {
        atomicAdd(&cover_long->n_reads, 1ull);
        atomicAdd(&cover_long->n_segs, (unsigned long long)flx_cover_seg_count(L, seg_bases));
    }
}

__global__ void k_widen_u32_i64(uint64_t n, const uint32_t *in, int64_t *out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = (int64_t)in[i];
}

// the ranges MODE 3 left inline -> their places in the CSR (+ every child's read); counts the reads that have more than fit inline
__global__ void __launch_bounds__(256) k_children_from_inline(uint64_t n, const uint32_t *n_child, const uint64_t *child_offsets, const int32_t *inline_ranges,
                                                              int32_t *child_ranges, uint32_t *child_parent, unsigned int *overflow,
                                                              const int32_t *lengths, int long_min) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t nc = n_child[i];
    if (nc == 0) return;
    if (long_min > 0 && lengths[i] >= long_min) return;  // a long read: the cooperative path writes its ranges, however many
    if (nc > (uint32_t)kInlineChildren) {
        atomicAdd(overflow, 1u);
        return;
    }
    const uint64_t at = child_offsets[i];
    const int32_t *src = inline_ranges + (size_t)i * kInlineChildren * 2;
    for (uint32_t k = 0; k < nc; ++k) {
        child_ranges[2 * (at + k)] = src[2 * k];
        child_ranges[2 * (at + k) + 1] = src[2 * k + 1];
        child_parent[at + k] = (uint32_t)i;
    }
}

// sort key of a child: longest first (the lanes of a wave then run the same number of steps)
__global__ void k_child_keys(uint64_t n, const int32_t *ranges, uint64_t *keys, uint32_t *vals) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        keys[i] = (uint64_t)(0x7fffffffu - (uint32_t)(ranges[2 * i + 1] - ranges[2 * i]));
        vals[i] = (uint32_t)i;
    }
}

}  // namespace

// the fold kernels: with the LDS ring when it fits (R words per lane; 4 waves per workgroup up to R = 64, one wave up to R = 512),
// else (windows beyond ~15 000 positions) both streams from global memory
// The timing bracket of a fold launch says which form ran: flx_score_kmer_fold.m<MODE>.<ring<R> | global>.<fp | grid>.  Every name is
// a static string (the context keeps the pointer) and complete, so none is a prefix of another; flx_timing_get("flx_score_kmer_fold")
// still sums all of them — one bracket per launch, none nested, so that sum is the device time of the folds.
#define FLX_FOLD_NAMES_PATH(m, path) {"flx_score_kmer_fold.m" #m "." path ".fp", "flx_score_kmer_fold.m" #m "." path ".grid"}
#define FLX_FOLD_NAMES_MODE(m)                                                                                         \
    {FLX_FOLD_NAMES_PATH(m, "ring32"), FLX_FOLD_NAMES_PATH(m, "ring64"), FLX_FOLD_NAMES_PATH(m, "ring128"),            \
     FLX_FOLD_NAMES_PATH(m, "ring256"), FLX_FOLD_NAMES_PATH(m, "ring512"), FLX_FOLD_NAMES_PATH(m, "global")}
static const char *const kFoldTimingNames[7][6][2] = {FLX_FOLD_NAMES_MODE(0), FLX_FOLD_NAMES_MODE(1), FLX_FOLD_NAMES_MODE(2), FLX_FOLD_NAMES_MODE(3),
                                                      FLX_FOLD_NAMES_MODE(4), FLX_FOLD_NAMES_MODE(5), FLX_FOLD_NAMES_MODE(6)};
#undef FLX_FOLD_NAMES_MODE
#undef FLX_FOLD_NAMES_PATH

template <int MODE>
static int launch_fold(flx_ctx *ctx, FoldArgs &a) {
    int R = 32, path = 0;  // path: 0..4 = the ring of 32 << path words, 5 = global streams
    while (R < (MODE == 6 ? 24 : 18) + (a.ws + 31) / 32) R *= 2, ++path;  // MODE 6 starts up to 4 words into its first block, and reads one word further
    const char *env = getenv("FLX_KMER_FOLD_STREAMS");  // "global": the round-2 data path (second implementation, tests)
    const bool ring = R <= 512 && !(env && strcmp(env, "global") == 0);
    if (!ring) path = 5;
    const unsigned threads = (!ring || R <= 64) ? 256u : 64u;
    const unsigned nb = (unsigned)(((MODE == 6 ? a.n_children : a.n_reads) + threads - 1) / threads);
    a.ring_words = R;
    const bool grid = ring && a.grid && !a.events && (MODE == 0 || MODE == 3 || MODE == 6);  // the steady state on the integer grid (GridTab)
    if (grid) {
        constexpr int M = (MODE == 0 || MODE == 3 || MODE == 6) ? MODE : 0;
        ctx->last_kmer_fold_grid = true;
        const size_t lds = (size_t)(threads / 64) * (size_t)R * 256 + 2048 * FLX_FOLD_WALK_COPIES + 1024;
        FLX_HIP(ctx, hipFuncSetAttribute((const void *)k_kmer_fold<M, true, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        flx_time_scope tf(ctx, kFoldTimingNames[MODE][path][1]);
        hipLaunchKernelGGL((k_kmer_fold<M, true, true>), dim3(nb), dim3(threads), lds, ctx->stream, a);
    } else if (ring) {
        const size_t lds = (size_t)(threads / 64) * (size_t)R * 256;
        FLX_HIP(ctx, hipFuncSetAttribute((const void *)k_kmer_fold<MODE, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        flx_time_scope tf(ctx, kFoldTimingNames[MODE][path][0]);
        hipLaunchKernelGGL((k_kmer_fold<MODE, true>), dim3(nb), dim3(threads), lds, ctx->stream, a);
    } else {
        flx_time_scope tf(ctx, kFoldTimingNames[MODE][path][0]);
        hipLaunchKernelGGL((k_kmer_fold<MODE, false>), dim3(nb), dim3(threads), 0, ctx->stream, a);
    }
    FLX_HIP(ctx, hipGetLastError());  // (a launch that fails must not pass for a kernel that wrote nothing)
    return FLX_OK;
}

int flx_score_kmer_dev(flx_ctx *ctx, const flx_kmerset *set, const uint8_t *d_plane, uint64_t plane_bytes,
                       const uint64_t *d_offsets, const int32_t *d_lengths, const uint32_t *d_order,
                       uint64_t n_reads, const flx_params *params, flx_scores *out) {
    out->n_children = 0;
    ctx->last_kmer_redo = nullptr;  // (they name workspace 0 of the previous call: not past the first return of this one)
    ctx->last_kmer_redo_n = 0;
    ctx->last_kmer_cover = "";
    if (n_reads == 0) return FLX_OK;
    hipStream_t st = ctx->stream;
    const bool want_children = params->trim || params->split_set;
    if (want_children && !out->child_offsets)
        return flx_fail(ctx, FLX_ERR_INVALID, "trim/split requested but child_offsets is NULL");
    const unsigned nb = (unsigned)((n_reads + 255) / 256);

    // ---- coverage plane layout: row i = ceil(L/8) bytes rounded up to 16, rows packed by an exclusive scan ----
    // All device memory of this path comes from the context's two grow-only workspaces: nothing is allocated or freed per
    // batch once they have reached their size.
    const size_t scan_ws = flx_radix_sort_workspace(n_reads + 1);
    auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const char *fold_env0 = getenv("FLX_KMER_FOLD");
    const bool inline_children = want_children && !(params->split_set && params->split < 32) && !fold_env0;  // (the one-lane-per-child path)
    // The cooperative path for ultra-long reads and children (score_kmer_long.hip) applies where the one-lane kernels would fold on
    // the integer grid: a window size whose grid table pays, none of the test-only fold variants, --split absent or >= 32.
    GridTab gt;
    const bool grid_pays = build_grid_table(params->window_size, gt);
    bool grid_on, events_on;
    {
        const char *ev_env = getenv("FLX_KMER_FOLD_EVENTS");
        events_on = ev_env && ev_env[0] == '1';
        const char *grid_env = getenv("FLX_KMER_FOLD_GRID");  // "0": the floating-point steady state (the second implementation; tests, A/B)
        grid_on = grid_pays && !(grid_env && grid_env[0] == '0');
    }
    KmerLong kl;
    FLX_CHECK(flx_kmer_long_threshold(ctx, plane_bytes, grid_on && !events_on && !fold_env0 && !(params->split_set && params->split < 32), &kl));
    // The cooperative path of the coverage stage (cover_long.hip): long reads are covered as segments, one wave each, by the
    // wave-level kernels — whatever the window size, --split and the fold variant; the workgroup-per-read form keeps them in its own launch
    CoverLong cvl;
    FLX_CHECK(flx_cover_long_threshold(ctx, plane_bytes, !flx_kmer_cover_is_v2(set), &cvl));
    const size_t small_bytes = 2 * up((n_reads + 1) * 8) + 3 * up(n_reads * 4) + up((n_reads + 1) * 4) + up(scan_ws) + up(n_reads) +
                               (inline_children ? up(n_reads * (size_t)kInlineChildren * 8) + up(64) : 0) + up(64);
    void *small = nullptr;
    FLX_CHECK(flx_workspace(ctx, 0, small_bytes, &small));
    char *wp = (char *)small;
    auto carve = [&](size_t bytes) { void *q = wp; wp += up(bytes); return q; };
    int64_t *d_rowb = (int64_t *)carve((n_reads + 1) * 8);
    int64_t *d_covoff = (int64_t *)carve((n_reads + 1) * 8);
    int32_t *d_cnt = (int32_t *)carve(n_reads * 4);
    int32_t *d_first_tmp = (int32_t *)carve(n_reads * 4);
    int32_t *d_last_tmp = (int32_t *)carve(n_reads * 4);
    uint32_t *d_nchild = (uint32_t *)carve((n_reads + 1) * 4);
    void *d_scanws = carve(scan_ws);
    uint8_t *d_redo = (uint8_t *)carve(n_reads);  // cover_queue.hip: marks of the reads handed to the kernel with a diagonal per lane
    int32_t *d_inline = inline_children ? (int32_t *)carve(n_reads * (size_t)kInlineChildren * 8) : nullptr;
    unsigned int *d_overflow = inline_children ? (unsigned int *)carve(64) : nullptr;
    int32_t *first = out->first ? out->first : d_first_tmp, *last = out->last ? out->last : d_last_tmp;
    // the counters of the cooperative paths, 64 bytes: the long reads' and (at + 1) the long children's counts for the folds, then
    // the coverage stage's long reads and segments — zeroed by one memset, read back by one copy with the wait below
    struct LongCounters {
        KmerLongCounts reads, children;
        CoverLongCounts cover;
    };
    static_assert(sizeof(LongCounters) == 64, "the counters' block");
    LongCounters *d_counters = (LongCounters *)carve(64);
    kl.d_reads = &d_counters->reads;
    kl.d_children = &d_counters->children;
    FLX_HIP(ctx, hipMemsetAsync(d_rowb, 0, (n_reads + 1) * 8, st));
    if (kl.on || cvl.on) FLX_HIP(ctx, hipMemsetAsync(d_counters, 0, sizeof(LongCounters), st));
    hipLaunchKernelGGL(k_cov_row_bytes, dim3(nb), dim3(256), 0, st, n_reads, d_lengths, d_rowb, kl.on ? kl.thr : 0, params->window_size, kl.d_reads,
                       cvl.on ? cvl.thr : 0, cvl.spans * 1024, &d_counters->cover);
    FLX_CHECK(flx_exclusive_scan_i64(ctx, n_reads + 1, d_rowb, d_covoff, d_scanws, scan_ws));
    int64_t cov_bytes = 0;
    KmerLongCounts long_reads = {0, 0}, long_children = {0, 0};
    LongCounters counters;
    memset(&counters, 0, sizeof counters);
    FLX_HIP(ctx, hipMemcpyAsync(&cov_bytes, d_covoff + n_reads, 8, hipMemcpyDeviceToHost, st));
    if (kl.on || cvl.on) FLX_HIP(ctx, hipMemcpyAsync(&counters, d_counters, sizeof counters, hipMemcpyDeviceToHost, st));  // (with the wait below)
    FLX_HIP(ctx, hipStreamSynchronize(st));
    long_reads = counters.reads;
    cvl.n = counters.cover;
    void *d_cov = nullptr;
    const size_t cov_room = up((size_t)cov_bytes + 64), long_room = long_reads.n ? flx_kmer_long_reads_workspace(long_reads) : 0;
    const size_t cover_long_room = cvl.n.n_segs ? flx_cover_long_workspace(cvl.n) : 0;
    const size_t cover_long_at = up(cov_room + long_room);
    FLX_CHECK(flx_workspace(ctx, 1, cover_long_at + cover_long_room, &d_cov));
    void *d_long_reads = long_reads.n ? (char *)d_cov + cov_room : nullptr, *d_long_children = nullptr;
    void *d_cover_long = cvl.n.n_segs ? (char *)d_cov + cover_long_at : nullptr;

    // ---- stage 1: lookups -> coverage bits (cover_common.h) ----
    FLX_CHECK(flx_kmer_cover_stage(ctx, set, d_plane, d_offsets, d_lengths, d_order, n_reads, (uint32_t *)d_cov, (const uint64_t *)d_covoff, d_cnt, first, last,
                                   d_redo, cvl, &d_counters->cover, d_cover_long, cover_long_room));

    // ---- stage 2: serial fold ----
    FoldArgs a;
    a.cov = (uint32_t *)d_cov;
    a.cov_off = (const uint64_t *)d_covoff;
    a.lengths = d_lengths;
    a.order = d_order;
    a.n_reads = n_reads;
    a.count = d_cnt;
    a.first = first;
    a.last = last;
    a.ws = params->window_size;
    a.ws_d = (double)(size_t)params->window_size;
    {
        volatile double one = 1.0, half = 0.5, wsd = a.ws_d;
        a.delta = one / wsd;
        a.clamp = half / wsd;
    }
    a.p = *params;
    a.gt = gt;
    a.events = events_on;
    a.grid = grid_on;
    a.long_min = kl.on ? kl.thr : 0;
    ctx->last_kmer_fold_grid = false;  // (launch_fold says so when a grid kernel really runs)
    a.mean_q = out->mean_q;
    a.window_q = out->window_q;
    a.passed = out->passed;
    a.n_child = nullptr;
    a.inline_ranges = d_inline;
    a.child_parent = nullptr;
    a.child_order = nullptr;
    a.n_children = 0;
    a.child_offsets = nullptr;
    a.child_ranges = out->child_ranges;
    a.child_mean_q = out->child_mean_q;
    a.child_window_q = out->child_window_q;
    a.child_passed = out->child_passed;

    // (every fold launch opens its own timing bracket: launch_fold)
    if (!want_children) {
        FLX_CHECK(launch_fold<0>(ctx, a));
        if (long_reads.n) FLX_CHECK(flx_kmer_long_reads(ctx, a, &kl, long_reads, false, d_long_reads, long_room));
        if (out->child_offsets) FLX_HIP(ctx, hipMemsetAsync(out->child_offsets, 0, (n_reads + 1) * 8, st));
        FLX_HIP(ctx, hipGetLastError());
        FLX_HIP(ctx, hipStreamSynchronize(st));
        flx_cover_long_report(cvl);
        return flx_kmer_long_report(ctx, kl, d_long_reads, nullptr);
    }

    FLX_HIP(ctx, hipMemsetAsync(d_nchild, 0, (n_reads + 1) * 4, st));
    a.n_child = d_nchild;
    // FLX_KMER_FOLD=bits forces the bit-level passes (tests compare the two implementations on every read)
    const char *fold_env = getenv("FLX_KMER_FOLD");
    const bool bit_level = (params->split_set && params->split < 32) || (fold_env && strcmp(fold_env, "bits") == 0);
    if (bit_level)
        FLX_CHECK(launch_fold<1>(ctx, a));  // runs inside one word can be bad ranges
    else
        FLX_CHECK(launch_fold<3>(ctx, a));
    // the long reads: their folds, their n_child, and how many of their children are long themselves
    if (long_reads.n) FLX_CHECK(flx_kmer_long_reads(ctx, a, &kl, long_reads, true, d_long_reads, long_room));
    // child_offsets = exclusive scan of the counts (n + 1 entries; the last one is the total)
    hipLaunchKernelGGL(k_widen_u32_i64, dim3((unsigned)((n_reads + 1 + 255) / 256)), dim3(256), 0, st, n_reads + 1,
                       d_nchild, d_rowb);
    FLX_CHECK(flx_exclusive_scan_i64(ctx, n_reads + 1, d_rowb, (int64_t *)out->child_offsets, d_scanws, scan_ws));
    int64_t total_children = 0;
    FLX_HIP(ctx, hipMemcpyAsync(&total_children, (int64_t *)out->child_offsets + n_reads, 8, hipMemcpyDeviceToHost, st));
    if (long_reads.n) FLX_HIP(ctx, hipMemcpyAsync(&long_children, kl.d_children, sizeof long_children, hipMemcpyDeviceToHost, st));
    FLX_HIP(ctx, hipStreamSynchronize(st));
    out->n_children = (uint64_t)total_children;
    if ((uint64_t)total_children > out->child_capacity)
        return flx_fail(ctx, FLX_ERR_CAPACITY, "child outputs need room for %lld children (capacity %llu)",
                        (long long)total_children, (unsigned long long)out->child_capacity);
    if (total_children > 0) {
        a.child_offsets = out->child_offsets;
        // FLX_KMER_FOLD=words: the children inside their read's lane (MODE 4, second implementation of the word-level path)
        const bool per_child = !bit_level && !(fold_env && strcmp(fold_env, "words") == 0);
        if (bit_level) {
            FLX_CHECK(launch_fold<2>(ctx, a));
        } else if (!per_child) {
            FLX_CHECK(launch_fold<4>(ctx, a));
        } else {
            // ranges (word-level events only) -> children by descending length -> one lane per child
            const uint64_t nc = (uint64_t)total_children;
            const size_t sort_ws = flx_radix_sort_workspace(nc);
            void *cw = nullptr;
            const size_t long_child_room = long_reads.n ? flx_kmer_long_children_workspace(long_children) : 0;
            FLX_CHECK(flx_workspace(ctx, 2, 2 * up(nc * 8) + 3 * up(nc * 4) + up(sort_ws) + long_child_room, &cw));
            wp = (char *)cw;
            uint64_t *keys0 = (uint64_t *)carve(nc * 8), *keys1 = (uint64_t *)carve(nc * 8);
            uint32_t *vals0 = (uint32_t *)carve(nc * 4), *vals1 = (uint32_t *)carve(nc * 4);
            a.child_parent = (uint32_t *)carve(nc * 4);
            void *d_sortws = carve(sort_ws);
            if (long_reads.n) d_long_children = carve(long_child_room);
            a.n_children = nc;
            unsigned int overflow = 1;
            if (d_inline) {  // the ranges MODE 3 left inline go to their places; a read with more than fit sends the batch through MODE 5
                FLX_HIP(ctx, hipMemsetAsync(d_overflow, 0, 4, st));
                {
                    flx_time_scope ti(ctx, "flx_score_kmer_fold.inline");  // (part of the folds' device time; closed before the host waits)
                    hipLaunchKernelGGL(k_children_from_inline, dim3(nb), dim3(256), 0, st, n_reads, (const uint32_t *)d_nchild, (const uint64_t *)out->child_offsets,
                                       (const int32_t *)d_inline, out->child_ranges, a.child_parent, d_overflow, d_lengths, a.long_min);
                }
                FLX_HIP(ctx, hipMemcpyAsync(&overflow, d_overflow, 4, hipMemcpyDeviceToHost, st));
                FLX_HIP(ctx, hipStreamSynchronize(st));
            }
            if (overflow) FLX_CHECK(launch_fold<5>(ctx, a));
            // the long reads' ranges, and the folds of the children that are long themselves (MODE 6 below leaves those alone)
            if (long_reads.n) FLX_CHECK(flx_kmer_long_children(ctx, a, &kl, long_reads, long_children, d_long_reads, d_long_children, long_child_room));
            hipLaunchKernelGGL(k_child_keys, dim3((unsigned)((nc + 255) / 256)), dim3(256), 0, st, nc, out->child_ranges, keys0, vals0);
            uint64_t *skeys = nullptr;
            uint32_t *svals = nullptr;
            FLX_CHECK(flx_radix_sort_pairs(ctx, nc, keys0, keys1, vals0, vals1, d_sortws, sort_ws, &skeys, &svals));
            a.child_order = svals;
            FLX_CHECK(launch_fold<6>(ctx, a));
        }
    }
    FLX_HIP(ctx, hipGetLastError());
    FLX_HIP(ctx, hipStreamSynchronize(st));
    flx_cover_long_report(cvl);
    return flx_kmer_long_report(ctx, kl, d_long_reads, d_long_children);
}
