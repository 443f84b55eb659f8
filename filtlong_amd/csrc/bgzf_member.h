// bgzf_member.h — the BGZF member encoder of bgzf.hip, one workgroup per member, written as barrier-free phases.
//
// Every phase is a function of (thread, shared state) with no barrier inside; k_bgzf_members (bgzf.hip) runs the phases
// in order with __syncthreads() between them.  The same functions compile for the host (the atomics below fall back to
// plain operations), so a serial walk over the threads of each phase reproduces the kernel's bytes exactly.
//
// Member k holds input bytes [k*65280, min(n, (k+1)*65280)) (bgzip's BGZF_BLOCK_SIZE).  Its BG_NT threads own BG_NT equal
// segments of the member.  The steps:
//   load     the member into LDS (data), the CRC table, x^(2^k) mod P, an empty hash table;
//   crc      each thread the CRC-32 of its segment from state 0; shifted by x^(8*bytes after it) and XORed, they give the
//            member's CRC (the polynomial arithmetic of zlib's crc32_combine);
//   match    rounds of BG_NT positions in input order: every position looks up the newest earlier position with the same
//            4-byte hash (head[], filled by atomicMax in the rounds before: deterministic, max does not depend on order),
//            checks the bytes, keeps the match if it is >= 4 long and <= 32768 back; then the round inserts its positions;
//   parse    each thread greedily over its own segment (matches cut at the segment's end), histograms by LDS atomics;
//   huffman  codes from the histograms (Moffat-Katajainen lengths, limited to 15 / 7 bits by the Kraft repair of the
//            per-length counts), the code-length header with the RLE symbols 16/17/18;
//   size     one dynamic block against one stored block: stored when it is not larger;
//   pack     each thread walks its segment again for its bit count, a scan gives its first bit, the bits go to the
//            member's output slot as 32-bit words: plain stores for the words a thread owns, atomicOr for the (zeroed)
//            words it shares with a neighbour.
#pragma once

#include <stdint.h>

#if defined(__HIP_DEVICE_COMPILE__)
#define BG_FN __device__ __forceinline__
#define BG_ATOMIC_MAX(p, v) atomicMax((p), (v))
#define BG_ATOMIC_ADD(p, v) atomicAdd((p), (v))
#define BG_ATOMIC_OR(p, v) atomicOr((p), (v))
#define BG_CLZ(x) __clz((int)(x))
#else
#if defined(__HIPCC__)
#define BG_FN __host__ __device__ inline
#else
#define BG_FN inline
#endif
#define BG_ATOMIC_MAX(p, v) (*(p) = (*(p) > (v) ? *(p) : (v)))
#define BG_ATOMIC_ADD(p, v) (*(p) += (v))
#define BG_ATOMIC_OR(p, v) (*(p) |= (v))
#define BG_CLZ(x) __builtin_clz(x)
#endif

namespace bgzf {

constexpr int BG_NT = 512;                 // threads per member (one workgroup)
constexpr uint32_t BG_MEMBER = 65280;      // input bytes per member (0xff00)
constexpr int BG_HBITS = 13;               // hash table: 8192 newest positions
constexpr uint32_t BG_DEFL_OFF = 32;       // the deflate stream starts at this (word-aligned) byte of a slot ...
constexpr uint32_t BG_SLOT = 65664;        // ... whose stride is this: 32 + (65280 + 5) + 8 <= 65664
constexpr uint32_t BG_MAX_DIST = 32768;
constexpr int BG_MIN_MATCH = 4;            // the hash covers 4 bytes
constexpr uint32_t BG_POLY = 0xedb88320u;

struct Shared {
    uint8_t data[BG_MEMBER + 16];          // the member (zero padded)
    int32_t head[1 << BG_HBITS];           // newest earlier position per hash, -1: none
    uint32_t crc_tab[256];
    uint32_t x2n[32];                      // x^(2^k) mod P (reflected)
    uint32_t part[BG_NT];                  // per segment: shifted CRC, then bit count, then first bit
    uint32_t hist_l[288], hist_d[32], hist_c[19];
    uint32_t sk[288];                      // Huffman: sorted keys (frequency, then code length) ...
    uint16_t ss[288];                      // ... and their symbols; lit/len in [0, 286), dist in sk_d/ss_d
    uint32_t sk_d[32];
    uint16_t ss_d[32];
    uint8_t len_l[288], len_d[32], len_c[19];
    uint16_t code_l[288], code_d[32], code_c[19];  // bit-reversed canonical codes
    uint16_t rle[320];                     // code-length symbols of the header: sym | extra << 8
    int n_rle, hlit, hdist, hclen;
    uint32_t hdr_bits;                     // 3 + 14 + 3*hclen + coded lengths
    uint32_t data_bits_l, data_bits_d;     // sum of freq * (length + extra bits)
    uint32_t crc;
    int stored;
    uint32_t defl_bytes;
};

BG_FN uint32_t seg_lo(int t, uint32_t n) { return (uint32_t)(((uint64_t)t * n) / BG_NT); }

BG_FN uint32_t multmodp(uint32_t a, uint32_t b) {  // a * b mod P, reflected (zlib crc32.c)
    uint32_t m = 1u << 31, p = 0;
    for (;;) {
        if (a & m) {
            p ^= b;
            if ((a & (m - 1)) == 0) break;
        }
        m >>= 1;
        b = (b & 1) ? (b >> 1) ^ BG_POLY : b >> 1;
    }
    return p;
}

BG_FN uint32_t x8nmodp(const Shared &S, uint32_t n) {  // x^(8n) mod P
    uint32_t p = 1u << 31;
    int k = 3;
    while (n) {
        if (n & 1) p = multmodp(S.x2n[k & 31], p);
        n >>= 1;
        ++k;
    }
    return p;
}

BG_FN uint32_t ilog2(uint32_t x) { return 31u - (uint32_t)BG_CLZ(x); }

// deflate's length symbol (257..285) and extra bits of a match length 3..258
BG_FN void len_sym(uint32_t L, uint32_t &sym, uint32_t &ne, uint32_t &ev) {
    if (L == 258) { sym = 285; ne = 0; ev = 0; return; }
    const uint32_t l = L - 3;
    ne = l < 8 ? 0 : ilog2(l) - 2;
    sym = 257 + 4 * ne + (l >> ne);
    ev = l & ((1u << ne) - 1);
}
// distance symbol (0..29) and extra bits of a distance 1..32768
BG_FN void dist_sym(uint32_t D, uint32_t &sym, uint32_t &ne, uint32_t &ev) {
    const uint32_t d = D - 1;
    ne = d < 2 ? 0 : ilog2(d) - 1;
    sym = 2 * ne + (d >> ne);
    ev = d & ((1u << ne) - 1);
}
BG_FN uint32_t len_extra_of_sym(uint32_t s) { return (s < 265 || s == 285) ? 0 : (s - 261) / 4; }
BG_FN uint32_t dist_extra_of_sym(uint32_t s) { return s < 4 ? 0 : s / 2 - 1; }

// ---- load -------------------------------------------------------------------------------------------------------
BG_FN void ph_load(int t, Shared &S, const uint8_t *in, uint32_t n, bool aligned16) {
    const uint32_t n16 = aligned16 ? n / 16 : 0;
    for (uint32_t j = t; j < n16; j += BG_NT) {
        const uint4 v = ((const uint4 *)in)[j];
        *(uint4 *)(S.data + 16 * j) = v;
    }
    for (uint32_t j = 16 * n16 + t; j < n + 16; j += BG_NT) S.data[j] = j < n ? in[j] : 0;
    for (int j = t; j < (1 << BG_HBITS); j += BG_NT) S.head[j] = -1;
    for (int j = t; j < 288; j += BG_NT) S.hist_l[j] = 0;
    if (t < 32) S.hist_d[t] = 0;
    if (t < 19) S.hist_c[t] = 0;
    if (t < 256) {
        uint32_t c = (uint32_t)t;
        for (int k = 0; k < 8; ++k) c = (c & 1) ? (c >> 1) ^ BG_POLY : c >> 1;
        S.crc_tab[t] = c;
    }
    if (t == BG_NT - 1) {
        uint32_t p = 1u << 30;  // x^1
        S.x2n[0] = p;
        for (int k = 1; k < 32; ++k) S.x2n[k] = p = multmodp(p, p);
    }
}

// ---- CRC-32 -------------------------------------------------------------------------------------------------------
BG_FN void ph_crc(int t, Shared &S, uint32_t n) {
    const uint32_t lo = seg_lo(t, n), hi = seg_lo(t + 1, n);
    uint32_t c = 0;
    for (uint32_t j = lo; j < hi; ++j) c = S.crc_tab[(c ^ S.data[j]) & 0xff] ^ (c >> 8);
    S.part[t] = lo < hi ? multmodp(x8nmodp(S, n - hi), c) : 0;
}
BG_FN void ph_crc_final(int t, Shared &S, uint32_t n) {
    if (t != 0) return;
    uint32_t r = multmodp(x8nmodp(S, n), 0xffffffffu);
    for (int k = 0; k < BG_NT; ++k) r ^= S.part[k];
    S.crc = ~r;
}

// ---- match finding ------------------------------------------------------------------------------------------------
BG_FN uint32_t hash4(const Shared &S, uint32_t i) {
    const uint32_t v = (uint32_t)S.data[i] | ((uint32_t)S.data[i + 1] << 8) | ((uint32_t)S.data[i + 2] << 16) |
                       ((uint32_t)S.data[i + 3] << 24);
    return (v * 2654435761u) >> (32 - BG_HBITS);
}
// round `base`: position base + t looks up the positions of the rounds before; mt[i] = dist << 16 | len, 0: none
BG_FN void ph_lookup(int t, Shared &S, uint32_t n, uint32_t base, uint32_t *mt) {
    const uint32_t i = base + t;
    if (i >= n) return;
    uint32_t m = 0;
    if (i + BG_MIN_MATCH <= n) {
        const int32_t c = S.head[hash4(S, i)];
        if (c >= 0 && i - (uint32_t)c <= BG_MAX_DIST) {
            const uint32_t lim = n - i < 258 ? n - i : 258;
            uint32_t L = 0;
            while (L < lim && S.data[c + L] == S.data[i + L]) ++L;
            if (L >= (uint32_t)BG_MIN_MATCH) m = ((i - (uint32_t)c) << 16) | L;
        }
    }
    mt[i] = m;
}
BG_FN void ph_insert(int t, Shared &S, uint32_t n, uint32_t base) {
    const uint32_t i = base + t;
    if (i + BG_MIN_MATCH <= n) BG_ATOMIC_MAX(&S.head[hash4(S, i)], (int32_t)i);
}

// ---- parse (greedy, per segment) ----------------------------------------------------------------------------------
// calls f(kind, a, b): kind 0 literal a; kind 1 match of length a at distance b
template <class F>
BG_FN void walk_segment(int t, const Shared &S, uint32_t n, const uint32_t *mt, F &&f) {
    const uint32_t lo = seg_lo(t, n), hi = seg_lo(t + 1, n);
    uint32_t p = lo;
    while (p < hi) {
        const uint32_t m = mt[p];
        uint32_t L = m & 0xffff;
        if (L > hi - p) L = hi - p;
        if (L >= 3) {
            f(1, L, m >> 16);
            p += L;
        } else {
            f(0, S.data[p], 0);
            ++p;
        }
    }
}
BG_FN void ph_hist(int t, Shared &S, uint32_t n, const uint32_t *mt) {
    walk_segment(t, S, n, mt, [&](int kind, uint32_t a, uint32_t b) {
        if (kind == 0) {
            BG_ATOMIC_ADD(&S.hist_l[a], 1u);
        } else {
            uint32_t s, ne, ev;
            len_sym(a, s, ne, ev);
            BG_ATOMIC_ADD(&S.hist_l[s], 1u);
            dist_sym(b, s, ne, ev);
            BG_ATOMIC_ADD(&S.hist_d[s], 1u);
        }
    });
    if (t == 0) BG_ATOMIC_ADD(&S.hist_l[256], 1u);  // end of block
}

// ---- Huffman ------------------------------------------------------------------------------------------------------
// place the used symbols of a histogram in ascending (frequency, symbol) order: thread s ranks symbol s
BG_FN void rank_place(int s, const uint32_t *hist, int nsym, uint32_t *sk, uint16_t *ss) {
    if (s >= nsym || hist[s] == 0) return;
    const uint32_t f = hist[s];
    int r = 0;
    for (int k = 0; k < nsym; ++k) {
        const uint32_t g = hist[k];
        r += (g != 0) & ((g < f) | ((g == f) & (k < s)));
    }
    sk[r] = f;
    ss[r] = (uint16_t)s;
}
BG_FN int count_used(const uint32_t *hist, int nsym) {
    int u = 0;
    for (int k = 0; k < nsym; ++k) u += hist[k] != 0;
    return u;
}
// code lengths of the m used symbols (A ascending by frequency; in place: A[i] becomes a length), Moffat & Katajainen
BG_FN void minimum_redundancy(uint32_t *A, int m) {
    if (m == 0) return;
    if (m == 1) { A[0] = 1; return; }
    A[0] += A[1];
    int root = 0, leaf = 2, next;
    for (next = 1; next < m - 1; ++next) {
        if (leaf >= m || A[root] < A[leaf]) { A[next] = A[root]; A[root++] = (uint32_t)next; }
        else A[next] = A[leaf++];
        if (leaf >= m || (root < next && A[root] < A[leaf])) { A[next] += A[root]; A[root++] = (uint32_t)next; }
        else A[next] += A[leaf++];
    }
    A[m - 2] = 0;
    for (next = m - 3; next >= 0; --next) A[next] = A[A[next]] + 1;
    int avbl = 1, used = 0, dpth = 0;
    root = m - 2;
    next = m - 1;
    while (avbl > 0) {
        while (root >= 0 && (int)A[root] == dpth) { ++used; --root; }
        while (avbl > used) { A[next--] = (uint32_t)dpth; --avbl; }
        avbl = 2 * used;
        ++dpth;
        used = 0;
    }
}
// lengths <= maxlen for the m used symbols (sorted ascending in sk/ss), canonical bit-reversed codes for all nsym
BG_FN void build_code(uint32_t *sk, const uint16_t *ss, int m, int nsym, int maxlen, uint8_t *len, uint16_t *code) {
    for (int s = 0; s < nsym; ++s) len[s] = 0;
    minimum_redundancy(sk, m);
    uint32_t cnt[33];
    for (int k = 0; k <= 32; ++k) cnt[k] = 0;
    for (int i = 0; i < m; ++i) ++cnt[sk[i] > 32 ? 32 : sk[i]];
    if (m > 1) {  // Kraft repair: fold the overlong codes into maxlen, then lengthen the longest codes below it
        for (int k = maxlen + 1; k <= 32; ++k) { cnt[maxlen] += cnt[k]; cnt[k] = 0; }
        uint32_t total = 0;
        for (int k = maxlen; k > 0; --k) total += cnt[k] << (maxlen - k);
        while (total != (1u << maxlen)) {
            --cnt[maxlen];
            for (int k = maxlen - 1; k > 0; --k)
                if (cnt[k]) { --cnt[k]; cnt[k + 1] += 2; break; }
            --total;
        }
    }
    for (int k = 1, j = m; k <= maxlen; ++k)  // most frequent symbols (the end of the order) get the shortest codes
        for (uint32_t c = cnt[k]; c > 0; --c) len[ss[--j]] = (uint8_t)k;
    uint32_t nextc[17];
    uint32_t c = 0;
    uint32_t bl[17];
    for (int k = 0; k <= 16; ++k) bl[k] = 0;
    for (int s = 0; s < nsym; ++s) ++bl[len[s]];
    bl[0] = 0;
    for (int k = 1; k <= 16; ++k) { c = (c + bl[k - 1]) << 1; nextc[k] = c; }
    for (int s = 0; s < nsym; ++s) {
        const int L = len[s];
        if (!L) { code[s] = 0; continue; }
        uint32_t v = nextc[L]++, r = 0;
        for (int b = 0; b < L; ++b) { r = (r << 1) | (v & 1); v >>= 1; }
        code[s] = (uint16_t)r;
    }
}
BG_FN void ph_rank(int t, Shared &S) {
    if (t < 286) rank_place(t, S.hist_l, 286, S.sk, S.ss);
    else if (t >= 320 && t < 350) rank_place(t - 320, S.hist_d, 30, S.sk_d, S.ss_d);
}
// thread 0: lit/len code, thread 64 (another wave): distance code
BG_FN void ph_codes(int t, Shared &S) {
    if (t == 0) {
        build_code(S.sk, S.ss, count_used(S.hist_l, 286), 286, 15, S.len_l, S.code_l);
        uint32_t b = 0;
        for (int s = 0; s < 286; ++s) b += S.hist_l[s] * (S.len_l[s] + (s >= 257 ? len_extra_of_sym(s) : 0));
        S.data_bits_l = b;
    } else if (t == 64) {
        build_code(S.sk_d, S.ss_d, count_used(S.hist_d, 30), 30, 15, S.len_d, S.code_d);
        uint32_t b = 0;
        for (int s = 0; s < 30; ++s) b += S.hist_d[s] * (S.len_d[s] + dist_extra_of_sym(s));
        S.data_bits_d = b;
    }
}
BG_FN int cl_order(int i) {  // the order of the code-length code's lengths in the header
    const int o[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    return o[i];
}
// thread 0: the code-length header (RLE of the lit/len and distance lengths as one sequence), its code, the size decision
BG_FN void ph_header(int t, Shared &S, uint32_t n) {
    if (t != 0) return;
    int hlit = 286, hdist = 30;
    while (hlit > 257 && S.len_l[hlit - 1] == 0) --hlit;
    while (hdist > 1 && S.len_d[hdist - 1] == 0) --hdist;
    S.hlit = hlit;
    S.hdist = hdist;
    const int tot = hlit + hdist;
    auto at = [&](int i) -> int { return i < hlit ? S.len_l[i] : S.len_d[i - hlit]; };
    int nr = 0;
    for (int i = 0; i < tot;) {
        const int v = at(i);
        int r = 1;
        while (i + r < tot && at(i + r) == v) ++r;
        if (v == 0 && r >= 3) {
            const int k = r > 138 ? 138 : r;
            S.rle[nr++] = k >= 11 ? (uint16_t)(18 | ((k - 11) << 8)) : (uint16_t)(17 | ((k - 3) << 8));
            i += k;
        } else if (v != 0 && r >= 4) {
            S.rle[nr++] = (uint16_t)v;
            int k = r - 1 > 6 ? 6 : r - 1;
            S.rle[nr++] = (uint16_t)(16 | ((k - 3) << 8));
            i += 1 + k;
        } else {
            S.rle[nr++] = (uint16_t)v;
            ++i;
        }
    }
    S.n_rle = nr;
    for (int k = 0; k < 19; ++k) S.hist_c[k] = 0;
    for (int k = 0; k < nr; ++k) ++S.hist_c[S.rle[k] & 0xff];
    if (count_used(S.hist_c, 19) < 2) S.hist_c[S.hist_c[0] ? 1 : 0] = 1;  // keep the code-length code complete
    const int mc = count_used(S.hist_c, 19);
    uint32_t ck[19];
    uint16_t cs[19];
    for (int s = 0; s < 19; ++s) rank_place(s, S.hist_c, 19, ck, cs);
    build_code(ck, cs, mc, 19, 7, S.len_c, S.code_c);
    int hclen = 19;
    while (hclen > 4 && S.len_c[cl_order(hclen - 1)] == 0) --hclen;
    S.hclen = hclen;
    uint32_t hb = 3 + 5 + 5 + 4 + 3 * hclen;
    for (int k = 0; k < nr; ++k) {
        const int s = S.rle[k] & 0xff;
        hb += S.len_c[s] + (s == 16 ? 2 : s == 17 ? 3 : s == 18 ? 7 : 0);
    }
    S.hdr_bits = hb;
    const uint32_t bits = hb + S.data_bits_l + S.data_bits_d;
    const uint32_t dyn = (bits + 7) / 8;
    S.stored = dyn >= n + 5;
    S.defl_bytes = S.stored ? n + 5 : dyn;
}

// ---- packing ------------------------------------------------------------------------------------------------------
// the bits [b0, b1) of a member's stream, 32 bits at a time; words shared with a neighbour (zeroed before) by atomicOr
struct BitWriter {
    uint32_t *out;
    uint64_t acc;
    uint32_t nacc, word, b0, b1;
    BG_FN BitWriter(uint32_t *o, uint32_t lo, uint32_t hi) : out(o), acc(0), nacc(lo & 31), word(lo >> 5), b0(lo), b1(hi) {}
    BG_FN void emit(uint32_t v) {
        const bool shared_lo = (word == (b0 >> 5)) && (b0 & 31);
        const bool shared_hi = (word == (b1 >> 5)) && (b1 & 31);
        if (shared_lo || shared_hi) BG_ATOMIC_OR(&out[word], v);
        else out[word] = v;
        ++word;
    }
    BG_FN void put(uint32_t bits, uint32_t nb) {
        acc |= (uint64_t)bits << nacc;
        nacc += nb;
        while (nacc >= 32) {
            emit((uint32_t)acc);
            acc >>= 32;
            nacc -= 32;
        }
    }
    BG_FN void flush() {
        if (nacc > 0) emit((uint32_t)acc);  // (the writer started at bit nacc of the first word: acc holds those zeros)
        nacc = 0;
    }
};

BG_FN uint32_t seg_bits(int t, const Shared &S, uint32_t n, const uint32_t *mt) {
    uint32_t b = 0;
    walk_segment(t, S, n, mt, [&](int kind, uint32_t a, uint32_t d) {
        if (kind == 0) {
            b += S.len_l[a];
        } else {
            uint32_t s, ne, ev;
            len_sym(a, s, ne, ev);
            b += S.len_l[s] + ne;
            dist_sym(d, s, ne, ev);
            b += S.len_d[s] + ne;
        }
    });
    if (t == BG_NT - 1) b += S.len_l[256];
    return b;
}
BG_FN void ph_count(int t, Shared &S, uint32_t n, const uint32_t *mt) {
    if (!S.stored) S.part[t] = seg_bits(t, S, n, mt);
}
BG_FN void ph_scan(int t, Shared &S) {
    if (t != 0 || S.stored) return;
    uint32_t b = S.hdr_bits;
    for (int k = 0; k < BG_NT; ++k) {
        const uint32_t c = S.part[k];
        S.part[k] = b;
        b += c;
    }
}
// zero the words a segment (or the header, thread 0) shares with a neighbour; the stored block needs none
BG_FN void ph_zero(int t, Shared &S, uint8_t *slot) {
    if (S.stored) return;
    uint32_t *w = (uint32_t *)(slot + BG_DEFL_OFF);
    const uint32_t lo = S.part[t], hi = t + 1 < BG_NT ? S.part[t + 1] : S.hdr_bits + S.data_bits_l + S.data_bits_d;
    if (lo & 31) w[lo >> 5] = 0;
    if (hi & 31) w[hi >> 5] = 0;  // (segment 0's first word is also the header's last)
}
BG_FN void ph_pack(int t, Shared &S, uint32_t n, const uint32_t *mt, uint8_t *slot) {
    if (S.stored) {  // one stored block: header byte, LEN, NLEN, the bytes
        uint8_t *d = slot + BG_DEFL_OFF;
        if (t == 0) {
            d[0] = 1;
            d[1] = (uint8_t)n;
            d[2] = (uint8_t)(n >> 8);
            d[3] = (uint8_t)~n;
            d[4] = (uint8_t)(~n >> 8);
        }
        for (uint32_t j = t; j < n; j += BG_NT) d[5 + j] = S.data[j];
        return;
    }
    uint32_t *w = (uint32_t *)(slot + BG_DEFL_OFF);
    const uint32_t total = S.hdr_bits + S.data_bits_l + S.data_bits_d;
    const uint32_t lo = S.part[t], hi = t + 1 < BG_NT ? S.part[t + 1] : total;
    if (t == 0) {
        BitWriter h(w, 0, S.hdr_bits);
        h.put(1, 1);  // BFINAL
        h.put(2, 2);  // BTYPE 10
        h.put((uint32_t)(S.hlit - 257), 5);
        h.put((uint32_t)(S.hdist - 1), 5);
        h.put((uint32_t)(S.hclen - 4), 4);
        for (int k = 0; k < S.hclen; ++k) h.put(S.len_c[cl_order(k)], 3);
        for (int k = 0; k < S.n_rle; ++k) {
            const uint32_t s = S.rle[k] & 0xff, e = S.rle[k] >> 8;
            h.put(S.code_c[s], S.len_c[s]);
            if (s == 16) h.put(e, 2);
            else if (s == 17) h.put(e, 3);
            else if (s == 18) h.put(e, 7);
        }
        h.flush();
    }
    if (lo == hi) return;
    BitWriter bw(w, lo, hi);
    walk_segment(t, S, n, mt, [&](int kind, uint32_t a, uint32_t d) {
        if (kind == 0) {
            bw.put(S.code_l[a], S.len_l[a]);
        } else {
            uint32_t s, ne, ev;
            len_sym(a, s, ne, ev);
            bw.put(S.code_l[s], S.len_l[s]);
            if (ne) bw.put(ev, ne);
            dist_sym(d, s, ne, ev);
            bw.put(S.code_d[s], S.len_d[s]);
            if (ne) bw.put(ev, ne);
        }
    });
    if (t == BG_NT - 1) bw.put(S.code_l[256], S.len_l[256]);
    bw.flush();
}
// thread 0: the gzip header with the BC subfield, the trailer after the deflate bytes; the member's size
BG_FN void ph_frame(int t, Shared &S, uint32_t n, uint8_t *slot, uint32_t *size) {
    if (t != 0) return;
    const uint32_t msize = 26 + S.defl_bytes;
    const uint8_t h[18] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0,
                           (uint8_t)(msize - 1), (uint8_t)((msize - 1) >> 8)};
    for (int k = 0; k < 18; ++k) slot[k] = h[k];
    uint8_t *tr = slot + BG_DEFL_OFF + S.defl_bytes;
    for (int k = 0; k < 4; ++k) tr[k] = (uint8_t)(S.crc >> (8 * k));
    for (int k = 0; k < 4; ++k) tr[4 + k] = (uint8_t)(n >> (8 * k));
    *size = msize;
}

}  // namespace bgzf
