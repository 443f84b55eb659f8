// bgzf_inflate_member.h — the BGZF member decoder of bgzf_inflate.hip, one wave per member, written as barrier-free phases.
//
// Like bgzf_member.h: every phase is a function of (lane, shared state) with no barrier inside; k_bgzf_inflate runs the phases in
// order with a barrier between them, and inflate_member_host() below walks the lanes of each phase serially, so the host gives the
// kernel's bytes and status words exactly.
//
// A member is a gzip header, a raw deflate stream (RFC 1951) and the 8-byte trailer (CRC-32, ISIZE).  Huffman decoding is serial,
// so lane 0 decodes and the wave's other lanes move bytes.  The member's whole output (at most 64 KiB) lives in LDS; matches copy
// inside it, and it goes to global memory once, after its CRC-32 has been checked.  One round of the loop:
//   window    all lanes: the next 1 KiB of deflate data into LDS as aligned words (bytes outside the deflate range read as 0);
//   decode    lane 0: a block header (stored: LEN / NLEN; dynamic: the code lengths), or up to BI_BATCH tokens of the block.  A token
//             is checked where it is decoded: a literal needs room below ISIZE, a match needs dist <= bytes produced so far and
//             end <= ISIZE.  What the copy phases get is in bounds by construction;
//   tables    all lanes: the lookup tables of the block's two codes (clear, then fill — one phase each);
//   stored    all lanes: the bytes of a stored block from the input;
//   literals  lane k: the k-th literal of the batch to its place;
//   match     for every match of the batch in order, all lanes: out[dst + i] = out[dst - dist + i % dist].
// Then the CRC-32 (64 segments, combined as in bgzf_member.h) against the trailer, and the store.
//
// What bounds it: the bit reader counts the bits it hands out against 8 x the deflate bytes and the decoder stops with a status as
// soon as it has used more; every round consumes at least one bit or ends the member, and the loop is capped besides.  Table lookups
// take an index masked to the table's size, and an entry of 0 sends the symbol to the canonical walk (count[] / sym[] of the code),
// which ends after 15 bits with "no such code".  The decoder may reject what zlib accepts (a literal/length code with a single
// symbol, an empty code-length code); it accepts nothing zlib rejects.
#pragma once

#include <stdint.h>

#include "bgzf_member.h"  // multmodp, BG_POLY, BG_FN

namespace bgzf_inf {

using bgzf::multmodp;

constexpr int BI_NT = 64;                 // lanes per member (one wave)
constexpr uint32_t BI_MAX_OUT = 65536;    // a BGZF member holds at most this many bytes
constexpr int BI_WIN_WORDS = 256;         // deflate data in LDS per round: 1 KiB; a round uses at most 14 + 57 + 316 * 14 bits
                                          // (a dynamic header) or 64 * 48 bits (a batch), so a fresh window never runs out
constexpr int BI_BATCH = 64;              // tokens per round
constexpr int BI_LROOT = 10, BI_DROOT = 8;

enum Status : uint32_t {
    ST_OK = 0,
    ST_FRAME = 1,        // gzip header / sizes of the member
    ST_BTYPE = 2,        // block type 3
    ST_STORED = 3,       // LEN != ~NLEN
    ST_COUNTS = 4,       // HLIT > 286 or HDIST > 30
    ST_CL_CODE = 5,      // code-length code over-subscribed, incomplete or empty
    ST_CL_REPEAT = 6,    // repeat without a previous length, or beyond HLIT + HDIST; or a code-length symbol without a code
    ST_NO_EOB = 7,       // symbol 256 has no code
    ST_LIT_CODE = 8,     // literal/length code over-subscribed or incomplete
    ST_DIST_CODE = 9,    // distance code over-subscribed, or incomplete other than a single 1-bit code / no code
    ST_LIT_SYM = 10,     // no such literal/length code, or symbol 286 / 287
    ST_DIST_SYM = 11,    // no such distance code, or symbol 30 / 31
    ST_DIST_FAR = 12,    // distance beyond the member's first byte
    ST_OUT_FULL = 13,    // more than ISIZE bytes
    ST_IN_END = 14,      // the deflate data ran out
    ST_IN_SPARE = 15,    // the final block ends before the last byte in front of the trailer
    ST_ISIZE = 16,       // fewer than ISIZE bytes
    ST_CRC = 17,
    ST_ROUNDS = 18       // the round cap (cannot happen: every round consumes input)
};

enum Mode : int { M_HEADER = 0, M_BLOCK = 1, M_DONE = 2 };

struct Shared {
    uint8_t out[BI_MAX_OUT];
    uint32_t win[BI_WIN_WORDS];
    uint32_t ltab[1 << BI_LROOT], dtab[1 << BI_DROOT];  // bits << 16 | symbol; 0: not in the table
    uint16_t lsym[288], dsym[32];                        // symbols in canonical order
    uint16_t lcount[16], dcount[16];                     // codes per length
    uint16_t code[320];                                  // canonical code of each symbol (lit/len, then distance)
    uint8_t lens[320];
    int nlen, ndist;
    uint32_t lit_dst[BI_BATCH], mat_dst[BI_BATCH], mat[BI_BATCH];  // mat: length | distance << 16 (a distance of 32768 fits: u32)
    uint8_t lit[BI_BATCH];
    int n_lit, n_mat;
    uint32_t st_src, st_len, st_dst;  // stored block: bytes [st_src, st_src + st_len) of the deflate data to out[st_dst ...]
    int build;                        // the tables of lens[] are to be built
    uint32_t crc_tab[256], x2n[32], part[BI_NT];
    // the member
    uint32_t defl_at, defl_bytes, isize, crc_want, mis;  // mis: bytes between the aligned word in front and the deflate data
    // the decoder between the rounds
    uint32_t used_bits, produced;
    int mode, last;
    uint32_t status;
};

BG_FN uint32_t rd32(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }

// ---- init: the member's frame (lane 0), the CRC tables ---------------------------------------------------------------------------
// `m` is the member, `msize` its bytes, `want_out` the room the caller gave it (out_off[k+1] - out_off[k])
BG_FN void ph_init(int t, Shared &S, const uint8_t *m, uint32_t msize, uint64_t want_out) {
    for (int j = t; j < 256; j += BI_NT) {
        uint32_t c = (uint32_t)j;
        for (int k = 0; k < 8; ++k) c = (c & 1) ? (c >> 1) ^ bgzf::BG_POLY : c >> 1;
        S.crc_tab[j] = c;
    }
    if (t == BI_NT - 1) {
        uint32_t p = 1u << 30;
        S.x2n[0] = p;
        for (int k = 1; k < 32; ++k) S.x2n[k] = p = multmodp(p, p);
    }
    if (t != 0) return;
    S.status = ST_FRAME;
    S.mode = M_DONE;
    S.used_bits = 0; S.produced = 0; S.last = 0; S.build = 0;
    S.n_lit = 0; S.n_mat = 0; S.st_len = 0;
    S.defl_at = 0; S.defl_bytes = 0; S.isize = 0; S.crc_want = 0; S.mis = 0;
    if (msize < 18 + 8 || msize > 65536 || m[0] != 0x1f || m[1] != 0x8b || m[2] != 8) return;
    const uint32_t flg = m[3];
    if (flg & 0xe0) return;
    uint32_t p = 10;
    if (flg & 4) {
        const uint32_t xlen = (uint32_t)m[10] | (uint32_t)m[11] << 8;
        p = 12 + xlen;
        if (p > msize) return;
    }
    for (uint32_t f = 8; f <= 16; f <<= 1)
        if (flg & f) {
            while (p < msize && m[p]) ++p;
            ++p;
        }
    if (flg & 2) p += 2;
    if (p + 8 >= msize) return;  // (at least one byte of deflate data)
    const uint32_t isize = rd32(m + msize - 4);
    if (isize > BI_MAX_OUT || (uint64_t)isize != want_out) return;
    S.defl_at = p;
    S.defl_bytes = msize - 8 - p;
    S.isize = isize;
    S.crc_want = rd32(m + msize - 8);
    S.mis = (uint32_t)((uintptr_t)(m + p) & 3);
    S.status = ST_OK;
    S.mode = M_HEADER;
}

// ---- window: BI_WIN_WORDS aligned words from the reader's position -----------------------------------------------------------
// V = mis bytes in front + the deflate data is word-aligned in memory; the window's word 0 is the word of V the next bit lies in
BG_FN void ph_window(int t, Shared &S, const uint8_t *m) {
    if (S.mode == M_DONE) return;
    const uint32_t vend = S.mis + S.defl_bytes;                   // bytes of V
    const uint32_t w0 = (S.mis * 8 + S.used_bits) >> 5;
    const uint8_t *v = m + S.defl_at - S.mis;                     // word-aligned, inside the member's header
    for (int j = t; j < BI_WIN_WORDS; j += BI_NT) {
        const uint32_t b = (w0 + (uint32_t)j) * 4;                // first byte of the word in V
        uint32_t x = 0;
        if (b < vend) {                                           // the word ends inside the trailer at the latest
            x = *(const uint32_t *)(v + b);
            if (b < S.mis) x &= 0xffffffffu << (8 * (S.mis - b));
            if (b + 4 > vend) x &= 0xffffffffu >> (8 * (b + 4 - vend));
        }
        S.win[j] = x;
    }
}

// ---- the bit reader of lane 0 (LSB first) ------------------------------------------------------------------------------------
struct Bits {
    const uint32_t *win;
    uint64_t buf;
    int cnt;        // valid bits in buf
    int wi;         // next window word
    uint32_t used;  // bits handed out since the start of the deflate data
    BG_FN void open(const Shared &S) {
        win = S.win;
        const uint32_t vb = S.mis * 8 + S.used_bits;
        buf = (uint64_t)(win[0] >> (vb & 31));
        cnt = 32 - (int)(vb & 31);
        wi = 1;
        used = S.used_bits;
    }
    BG_FN int words_left() const { return BI_WIN_WORDS - wi; }
    BG_FN void refill() {  // more than 32 valid bits while the window lasts
        while (cnt <= 32 && wi < BI_WIN_WORDS) {
            buf |= (uint64_t)win[wi++] << cnt;
            cnt += 32;
        }
    }
    BG_FN uint32_t peek(int n) const { return (uint32_t)(buf & ((1ull << n) - 1)); }
    BG_FN void drop(int n) { buf >>= n; cnt -= n; used += (uint32_t)n; }
    BG_FN uint32_t get(int n) { const uint32_t v = peek(n); drop(n); return v; }
};

BG_FN uint32_t len_base(uint32_t s, uint32_t &ne) {  // s in 257..285
    if (s < 265) { ne = 0; return s - 254; }
    if (s == 285) { ne = 0; return 258; }
    ne = (s - 261) / 4;
    return 3 + ((4 + (s - 261) % 4) << ne);
}
BG_FN uint32_t dist_base(uint32_t s, uint32_t &ne) {  // s in 0..29
    if (s < 4) { ne = 0; return s + 1; }
    ne = s / 2 - 1;
    return 1 + ((2 + (s & 1)) << ne);
}

// Kraft sum of a code: 0 complete, > 0 incomplete, < 0 over-subscribed; *max = longest code (0: none); count[] per length
BG_FN int kraft(const uint8_t *lens, int n, uint16_t *count, int *max) {
    for (int k = 0; k < 16; ++k) count[k] = 0;
    for (int i = 0; i < n; ++i) ++count[lens[i]];
    count[0] = 0;
    int mx = 15;
    while (mx >= 1 && count[mx] == 0) --mx;
    *max = mx;
    int left = 1;
    for (int k = 1; k <= 15; ++k) {
        left <<= 1;
        left -= count[k];
        if (left < 0) return -1;
    }
    return left;
}
// canonical codes of the n symbols (code[]) and the symbols in canonical order (sym[])
BG_FN void canonical(const uint8_t *lens, int n, const uint16_t *count, uint16_t *code, uint16_t *sym) {
    uint32_t next[16], offs[16];
    uint32_t c = 0, o = 0;
    next[0] = 0; offs[0] = 0;
    for (int k = 1; k <= 15; ++k) {
        c = (c + (k > 1 ? count[k - 1] : 0)) << 1;
        next[k] = c;
        offs[k] = o;
        o += count[k];
    }
    for (int s = 0; s < n; ++s) {
        const int L = lens[s];
        code[s] = 0;
        if (!L) continue;
        code[s] = (uint16_t)next[L]++;
        sym[offs[L]++] = (uint16_t)s;
    }
}
// one symbol: the table, else the canonical walk; -1: no such code.  Needs 15 bits in the reader (zeros behind the data).
BG_FN int decode_sym(Bits &in, const uint32_t *tab, int root, const uint16_t *count, const uint16_t *sym) {
    const uint32_t e = tab[in.peek(root)];
    if (e) {
        in.drop((int)(e >> 16));
        return (int)(e & 0xffff);
    }
    int code = 0, first = 0, index = 0;
    for (int len = 1; len <= 15; ++len) {
        code |= (int)in.get(1);
        const int c = count[len];
        if (code - c < first) return sym[index + (code - first)];
        index += c;
        first += c;
        first <<= 1;
        code <<= 1;
    }
    return -1;
}

BG_FN void fail(Shared &S, uint32_t st) { S.status = st; S.mode = M_DONE; }

// the code lengths of a dynamic block (after its 3 header bits): S.lens, S.nlen, S.ndist; false: S.status is set
BG_FN bool dynamic_lengths(Shared &S, Bits &in) {
    in.refill();
    const int nlen = (int)in.get(5) + 257, ndist = (int)in.get(5) + 1, ncode = (int)in.get(4) + 4;
    if (nlen > 286 || ndist > 30) { fail(S, ST_COUNTS); return false; }
    uint8_t cll[19];
    for (int i = 0; i < 19; ++i) cll[i] = 0;
    for (int i = 0; i < ncode; ++i) {
        in.refill();
        cll[bgzf::cl_order(i)] = (uint8_t)in.get(3);
    }
    // the code-length code: 19 symbols of at most 7 bits, through the same canonical walk (no table: entry 0)
    uint16_t ccount[16], ccode[19], csym[19];
    int cmax;
    if (kraft(cll, 19, ccount, &cmax) != 0 || cmax == 0) { fail(S, ST_CL_CODE); return false; }
    canonical(cll, 19, ccount, ccode, csym);
    const uint32_t none = 0;
    int i = 0;
    while (i < nlen + ndist) {
        in.refill();
        const int sym = decode_sym(in, &none, 0, ccount, csym);
        if (sym < 0) { fail(S, ST_CL_REPEAT); return false; }
        if (sym < 16) { S.lens[i++] = (uint8_t)sym; continue; }
        int rep;
        uint8_t prev = 0;
        if (sym == 16) {
            if (i == 0) { fail(S, ST_CL_REPEAT); return false; }
            prev = S.lens[i - 1];
            rep = 3 + (int)in.get(2);
        } else if (sym == 17) {
            rep = 3 + (int)in.get(3);
        } else {
            rep = 11 + (int)in.get(7);
        }
        if (i + rep > nlen + ndist) { fail(S, ST_CL_REPEAT); return false; }
        while (rep--) S.lens[i++] = prev;  // (a run may cross from the literal/length lengths into the distance lengths)
        if (in.used > S.defl_bytes * 8) { fail(S, ST_IN_END); return false; }
    }
    if (in.used > S.defl_bytes * 8) { fail(S, ST_IN_END); return false; }
    S.nlen = nlen;
    S.ndist = ndist;
    return true;
}

// S.lens / nlen / ndist -> counts, canonical codes and orders; the completeness rules; S.build
BG_FN bool prepare_codes(Shared &S) {
    if (S.lens[256] == 0) { fail(S, ST_NO_EOB); return false; }
    int lmax, dmax;
    if (kraft(S.lens, S.nlen, S.lcount, &lmax) != 0) { fail(S, ST_LIT_CODE); return false; }
    const int dleft = kraft(S.lens + S.nlen, S.ndist, S.dcount, &dmax);
    if (dleft < 0 || (dleft > 0 && dmax > 1)) { fail(S, ST_DIST_CODE); return false; }  // (dmax 0: no code; dmax 1: one 1-bit code)
    canonical(S.lens, S.nlen, S.lcount, S.code, S.lsym);
    canonical(S.lens + S.nlen, S.ndist, S.dcount, S.code + S.nlen, S.dsym);
    S.build = 1;
    return true;
}

// ---- decode: lane 0 ----------------------------------------------------------------------------------------------------------
BG_FN void ph_decode(int t, Shared &S) {
    if (t != 0 || S.mode == M_DONE) return;
    S.n_lit = 0; S.n_mat = 0; S.st_len = 0; S.build = 0;
    const uint32_t avail = S.defl_bytes * 8;
    Bits in;
    in.open(S);
    if (S.mode == M_HEADER) {
        in.refill();
        S.last = (int)in.get(1);
        const uint32_t type = in.get(2);
        if (in.used > avail) { fail(S, ST_IN_END); return; }
        if (type == 3) { fail(S, ST_BTYPE); return; }
        if (type == 0) {
            in.drop((int)((8 - (in.used & 7)) & 7));  // to the byte boundary
            in.refill();
            const uint32_t len = in.get(16);
            in.refill();
            const uint32_t nlen = in.get(16);
            if (in.used > avail) { fail(S, ST_IN_END); return; }
            if ((len ^ nlen) != 0xffffu) { fail(S, ST_STORED); return; }
            const uint32_t src = in.used >> 3;
            if (len > S.defl_bytes - src) { fail(S, ST_IN_END); return; }
            if (len > S.isize - S.produced) { fail(S, ST_OUT_FULL); return; }
            S.st_src = src; S.st_len = len; S.st_dst = S.produced;
            S.produced += len;
            S.used_bits = (src + len) * 8;
            if (S.last) S.mode = M_DONE;
            return;
        }
        if (type == 1) {
            for (int i = 0; i < 144; ++i) S.lens[i] = 8;
            for (int i = 144; i < 256; ++i) S.lens[i] = 9;
            for (int i = 256; i < 280; ++i) S.lens[i] = 7;
            for (int i = 280; i < 288; ++i) S.lens[i] = 8;
            for (int i = 288; i < 320; ++i) S.lens[i] = 5;
            S.nlen = 288;
            S.ndist = 32;
        } else if (!dynamic_lengths(S, in)) {
            return;
        }
        if (!prepare_codes(S)) return;
        S.used_bits = in.used;
        S.mode = M_BLOCK;
        return;
    }
    // M_BLOCK: tokens until the batch is full, the block ends or the window runs low
    int nl = 0, nm = 0;
    uint32_t produced = S.produced;
    while (nl < BI_BATCH && nm < BI_BATCH && in.words_left() >= 2) {
        in.refill();
        const int s = decode_sym(in, S.ltab, BI_LROOT, S.lcount, S.lsym);
        if (s < 0 || s >= 286) { fail(S, ST_LIT_SYM); return; }
        if (in.used > avail) { fail(S, ST_IN_END); return; }
        if (s < 256) {
            if (produced >= S.isize) { fail(S, ST_OUT_FULL); return; }
            S.lit[nl] = (uint8_t)s;
            S.lit_dst[nl++] = produced++;
            continue;
        }
        if (s == 256) {
            S.mode = S.last ? M_DONE : M_HEADER;
            break;
        }
        uint32_t ne;
        uint32_t len = len_base((uint32_t)s, ne);
        len += in.get((int)ne);
        in.refill();
        const int d = decode_sym(in, S.dtab, BI_DROOT, S.dcount, S.dsym);
        if (d < 0 || d >= 30) { fail(S, ST_DIST_SYM); return; }
        uint32_t dist = dist_base((uint32_t)d, ne);
        dist += in.get((int)ne);
        if (in.used > avail) { fail(S, ST_IN_END); return; }
        if (dist > produced) { fail(S, ST_DIST_FAR); return; }
        if (len > S.isize - produced) { fail(S, ST_OUT_FULL); return; }
        S.mat[nm] = len | dist << 16;
        S.mat_dst[nm++] = produced;
        produced += len;
    }
    S.n_lit = nl; S.n_mat = nm;
    S.produced = produced;
    S.used_bits = in.used;
}

// ---- tables ------------------------------------------------------------------------------------------------------------------
BG_FN void ph_tables_clear(int t, Shared &S) {
    if (!S.build) return;
    for (int j = t; j < (1 << BI_LROOT); j += BI_NT) S.ltab[j] = 0;
    for (int j = t; j < (1 << BI_DROOT); j += BI_NT) S.dtab[j] = 0;
}
BG_FN void fill_code(uint32_t *tab, int root, uint32_t code, int len, uint32_t sym) {
    if (len == 0 || len > root) return;
    uint32_t rev = 0;
    for (int b = 0; b < len; ++b) rev |= ((code >> b) & 1u) << (len - 1 - b);
    const uint32_t e = (uint32_t)len << 16 | sym;
    for (uint32_t k = rev; k < (1u << root); k += 1u << len) tab[k] = e;  // (distinct codes fill distinct entries: prefix-free)
}
BG_FN void ph_tables_fill(int t, Shared &S) {
    if (!S.build) return;
    for (int s = t; s < S.nlen; s += BI_NT) fill_code(S.ltab, BI_LROOT, S.code[s], S.lens[s], (uint32_t)s);
    for (int s = t; s < S.ndist; s += BI_NT) fill_code(S.dtab, BI_DROOT, S.code[S.nlen + s], S.lens[S.nlen + s], (uint32_t)s);
}

// ---- moving bytes ------------------------------------------------------------------------------------------------------------
BG_FN void ph_stored(int t, Shared &S, const uint8_t *m) {
    const uint8_t *src = m + S.defl_at + S.st_src;
    for (uint32_t j = t; j < S.st_len; j += BI_NT) S.out[S.st_dst + j] = src[j];
}
BG_FN void ph_literals(int t, Shared &S) {
    for (int k = t; k < S.n_lit; k += BI_NT) S.out[S.lit_dst[k]] = S.lit[k];
}
BG_FN void ph_match(int t, Shared &S, int k) {
    const uint32_t len = S.mat[k] & 0xffff, dist = S.mat[k] >> 16, dst = S.mat_dst[k];
    const uint32_t from = dst - dist;
    for (uint32_t i = t; i < len; i += BI_NT) S.out[dst + i] = S.out[from + (dist >= len ? i : i % dist)];
}

// ---- the end: where the stream stopped, ISIZE, CRC-32 ------------------------------------------------------------------------
BG_FN void ph_end(int t, Shared &S) {
    if (t != 0 || S.status != ST_OK) return;
    if ((S.used_bits + 7) / 8 != S.defl_bytes) S.status = (S.used_bits + 7) / 8 > S.defl_bytes ? ST_IN_END : ST_IN_SPARE;
    else if (S.produced != S.isize) S.status = ST_ISIZE;
}
BG_FN uint32_t x8nmodp(const Shared &S, uint32_t n) {
    uint32_t p = 1u << 31;
    int k = 3;
    while (n) {
        if (n & 1) p = multmodp(S.x2n[k & 31], p);
        n >>= 1;
        ++k;
    }
    return p;
}
BG_FN uint32_t seg_lo(int t, uint32_t n) { return (uint32_t)(((uint64_t)t * n) / BI_NT); }
BG_FN void ph_crc(int t, Shared &S) {
    if (S.status != ST_OK) return;
    const uint32_t n = S.isize, lo = seg_lo(t, n), hi = seg_lo(t + 1, n);
    uint32_t c = 0;
    for (uint32_t j = lo; j < hi; ++j) c = S.crc_tab[(c ^ S.out[j]) & 0xff] ^ (c >> 8);
    S.part[t] = lo < hi ? multmodp(x8nmodp(S, n - hi), c) : 0;
}
BG_FN void ph_crc_final(int t, Shared &S) {
    if (t != 0 || S.status != ST_OK) return;
    uint32_t r = multmodp(x8nmodp(S, S.isize), 0xffffffffu);
    for (int k = 0; k < BI_NT; ++k) r ^= S.part[k];
    if (~r != S.crc_want) S.status = ST_CRC;
}

// ---- store: the member's bytes to their place (only when it is ok), its status word ---------------------------------------------
BG_FN void ph_store(int t, Shared &S, uint8_t *dst, uint32_t *status) {
    if (t == 0) *status = S.status;
    if (S.status != ST_OK) return;
    const uint32_t n = S.isize;
    uint32_t head = (uint32_t)((4 - ((uintptr_t)dst & 3)) & 3);
    if (head > n) head = n;
    const uint32_t words = (n - head) / 4;
    if ((uint32_t)t < head) dst[t] = S.out[t];
    for (uint32_t j = t; j < words; j += BI_NT) *(uint32_t *)(dst + head + 4 * j) = rd32(S.out + head + 4 * j);
    for (uint32_t j = head + 4 * words + t; j < n; j += BI_NT) dst[j] = S.out[j];
}

// the most rounds a member can take: every round but a "window ran low" one consumes a bit, and those come at most every other round
BG_FN uint32_t max_rounds(const Shared &S) { return 2 * (S.defl_bytes * 8 + 8); }

#if !defined(__HIP_DEVICE_COMPILE__)
// The kernel's loop on the host, the lanes of every phase in order.  `m`: the member (msize bytes); `dst`: want_out bytes.
inline uint32_t inflate_member_host(Shared &S, const uint8_t *m, uint32_t msize, uint64_t want_out, uint8_t *dst) {
#define BI_ALL(call) for (int t = 0; t < BI_NT; ++t) call
    BI_ALL(ph_init(t, S, m, msize, want_out));
    const uint32_t cap = max_rounds(S);
    for (uint32_t r = 0; S.mode != M_DONE; ++r) {
        if (r >= cap) { fail(S, ST_ROUNDS); break; }
        BI_ALL(ph_window(t, S, m));
        BI_ALL(ph_decode(t, S));
        BI_ALL(ph_tables_clear(t, S));
        BI_ALL(ph_tables_fill(t, S));
        BI_ALL(ph_stored(t, S, m));
        BI_ALL(ph_literals(t, S));
        for (int k = 0; k < S.n_mat; ++k) BI_ALL(ph_match(t, S, k));
    }
    BI_ALL(ph_end(t, S));
    BI_ALL(ph_crc(t, S));
    BI_ALL(ph_crc_final(t, S));
    uint32_t st = 0;
    BI_ALL(ph_store(t, S, dst, &st));
#undef BI_ALL
    return st;
}
#endif

}  // namespace bgzf_inf
