// deflate_markers.h — an RFC 1951 decoder that can start without its window: what a back-reference would have copied from in front
// of the starting point comes out as a marker, to be replaced once the window is known (the technique published with pugz /
// rapidgzip; pinflate_rounds.h says how the pieces are put together).  No zlib and no threads in here: bits in, 16-bit symbols out.
// The deflate format itself is RFC 1951; nothing here is taken from zlib's or the reference's sources.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

namespace pinflate {

struct Entry {
    uint16_t val;  // literal byte / base of a length or distance / offset of a secondary table
    uint8_t bits;  // bits this entry consumes
    uint8_t op;
};
enum : uint8_t { OP_LIT = 0, OP_EOB = 1, OP_LINK = 2, OP_BAD = 3, OP_BASE = 16 /* + number of extra bits */ };

static const uint16_t kLenBase[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
static const uint8_t kLenExtra[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
static const uint16_t kDistBase[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097,
                                       6145, 8193, 12289, 16385, 24577};
static const uint8_t kDistExtra[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};

// LSB-first bit reader over the mapped file
struct Bits {
    const uint8_t *base = nullptr, *end = nullptr, *p = nullptr;
    uint64_t buf = 0;
    int cnt = 0;  // valid bits in buf; negative: read past the end of the data
    void init(const uint8_t *data, size_t size) { base = data; end = data + size; }
    void seek(uint64_t bitpos) {
        p = base + (bitpos >> 3);
        buf = 0;
        cnt = 0;
        if (p > end) { p = end; cnt = -1; return; }
        refill();
        drop((int)(bitpos & 7));
    }
    uint64_t pos() const { return (uint64_t)(p - base) * 8 - (uint64_t)cnt; }
    inline void refill() {  // at least 56 valid bits afterwards (fewer only at the end of the data)
        if (p + 8 <= end) {
            uint64_t v;
            memcpy(&v, p, 8);
            buf |= v << cnt;
            p += (63 - cnt) >> 3;
            cnt |= 56;
        } else {
            while (cnt <= 56 && p < end) { buf |= (uint64_t)*p++ << cnt; cnt += 8; }
        }
    }
    inline void drop(int n) { buf >>= n; cnt -= n; }
    inline uint32_t peek(int n) const { return (uint32_t)(buf & ((1ull << n) - 1)); }
    inline uint32_t get(int n) { const uint32_t v = peek(n); drop(n); return v; }
};

// One canonical Huffman code as a two-level table: `root` bits index the primary table, longer codes continue in a secondary table
// of 2^(max - root) entries behind it.
struct Huff {
    enum Kind { CODES, LENS, DISTS };
    std::vector<Entry> t;
    int root = 0, sub = 0;
    uint32_t root_mask = 0, sub_mask = 0;

    // false: over-subscribed, or incomplete where the format does not allow it (RFC 1951 3.2.7; a single one-bit code is the exception
    // decoders accept for length and distance sets)
    bool build(const uint8_t *lens, int n, int root_bits, Kind kind) {
        int count[16] = {0};
        for (int i = 0; i < n; ++i) ++count[lens[i]];
        int max = 15;
        while (max >= 1 && count[max] == 0) --max;
        root = root_bits;
        root_mask = (1u << root) - 1;
        const Entry bad = {0, 1, OP_BAD};
        if (max == 0) {  // no code at all: every symbol is an error (a distance set may be empty when the block has no match)
            sub = 0; sub_mask = 0;
            t.assign((size_t)1 << root, bad);
            return true;
        }
        int left = 1;
        for (int len = 1; len <= 15; ++len) {
            left <<= 1;
            left -= count[len];
            if (left < 0) return false;
        }
        if (left > 0 && (kind == CODES || max != 1)) return false;
        sub = max > root ? max - root : 0;
        sub_mask = (1u << sub) - 1;
        t.assign((size_t)1 << root, bad);
        uint32_t next_code[16];
        uint32_t code = 0;
        count[0] = 0;
        for (int len = 1; len <= 15; ++len) {
            code = (code + (uint32_t)count[len - 1]) << 1;
            next_code[len] = code;
        }
        for (int sym = 0; sym < n; ++sym) {
            const int len = lens[sym];
            if (!len) continue;
            const uint32_t c = next_code[len]++;
            uint32_t rev = 0;
            for (int b = 0; b < len; ++b) rev |= ((c >> b) & 1u) << (len - 1 - b);
            Entry e;
            if (kind == CODES) {
                e = {(uint16_t)sym, 0, OP_LIT};
            } else if (kind == LENS) {
                if (sym < 256) e = {(uint16_t)sym, 0, OP_LIT};
                else if (sym == 256) e = {0, 0, OP_EOB};
                else if (sym < 286) e = {kLenBase[sym - 257], 0, (uint8_t)(OP_BASE + kLenExtra[sym - 257])};
                else e = {0, 0, OP_BAD};
            } else {
                if (sym < 30) e = {kDistBase[sym], 0, (uint8_t)(OP_BASE + kDistExtra[sym])};
                else e = {0, 0, OP_BAD};
            }
            if (len <= root) {
                e.bits = (uint8_t)len;
                for (uint32_t k = rev; k < (1u << root); k += 1u << len) t[k] = e;
            } else {
                const uint32_t prefix = rev & root_mask;
                if (t[prefix].op != OP_LINK) {
                    const size_t at = t.size();
                    if (at > 60000) return false;
                    t.resize(at + ((size_t)1 << sub), bad);
                    t[prefix] = {(uint16_t)at, (uint8_t)root, OP_LINK};
                }
                e.bits = (uint8_t)(len - root);
                const size_t at = t[prefix].val;
                for (uint32_t k = rev >> root; k < (1u << sub); k += 1u << (len - root)) t[at + k] = e;
            }
        }
        return true;
    }
    inline Entry decode(Bits &in) const {  // needs max <= 15 valid bits
        Entry e = t[in.buf & root_mask];
        if (e.op == OP_LINK) {
            in.drop(root);
            e = t[e.val + (in.buf & sub_mask)];
        }
        in.drop(e.bits);
        return e;
    }
};

static inline bool text_byte(unsigned c) { return c >= 32 ? c != 127 : (c == 9 || c == 10 || c == 13); }

enum Status { OK = 0, FAIL = 1, LIMIT = 2 };

// decoder of one thread: tables, the fixed code, the symbol output
struct Decoder {
    Bits in;
    Huff lit, dist, cl, fixed_lit, fixed_dist;
    bool have_fixed = false;
    std::vector<uint16_t> out;  // symbols: < 256 a byte, else 256 + index into the 32 KiB in front of the chunk
    size_t n = 0;               // symbols produced
    size_t limit = 0;           // give up beyond this many symbols

    void ensure_fixed() {
        if (have_fixed) return;
        uint8_t l[288];
        for (int i = 0; i < 144; ++i) l[i] = 8;
        for (int i = 144; i < 256; ++i) l[i] = 9;
        for (int i = 256; i < 280; ++i) l[i] = 7;
        for (int i = 280; i < 288; ++i) l[i] = 8;
        fixed_lit.build(l, 288, 10, Huff::LENS);
        uint8_t d[32];
        for (int i = 0; i < 32; ++i) d[i] = 5;
        fixed_dist.build(d, 32, 8, Huff::DISTS);
        have_fixed = true;
    }

    // the header of a dynamic block (after its three header bits): builds lit / dist
    bool dynamic_header() {
        in.refill();
        const int nlen = (int)in.get(5) + 257, ndist = (int)in.get(5) + 1, ncode = (int)in.get(4) + 4;
        if (nlen > 286 || ndist > 30) return false;
        static const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
        uint8_t cll[19] = {0};
        for (int i = 0; i < ncode; ++i) {
            if ((i & 7) == 0) in.refill();
            cll[order[i]] = (uint8_t)in.get(3);
        }
        if (in.cnt < 0) return false;
        if (!cl.build(cll, 19, 7, Huff::CODES)) return false;
        uint8_t lens[286 + 30];
        int i = 0;
        while (i < nlen + ndist) {
            in.refill();
            const Entry e = cl.decode(in);
            if (e.op != OP_LIT) return false;
            const int sym = e.val;
            if (sym < 16) { lens[i++] = (uint8_t)sym; continue; }
            int rep;
            uint8_t prev = 0;
            if (sym == 16) {
                if (i == 0) return false;
                prev = lens[i - 1];
                rep = 3 + (int)in.get(2);
            } else if (sym == 17) {
                rep = 3 + (int)in.get(3);
            } else {
                rep = 11 + (int)in.get(7);
            }
            if (i + rep > nlen + ndist) return false;
            while (rep--) lens[i++] = prev;
            if (in.cnt < 0) return false;
        }
        if (in.cnt < 0) return false;
        if (lens[256] == 0) return false;  // no end-of-block code
        return lit.build(lens, nlen, 10, Huff::LENS) && dist.build(lens + nlen, ndist, 8, Huff::DISTS);
    }

    // the symbols of one compressed block with the code sets l / d, up to its end-of-block code (the bit reader and the output
    // position are copied to locals: the loop keeps them in registers)
    Status block(const Huff &l, const Huff &d, bool check_text) { return check_text ? block_t<true>(l, d) : block_t<false>(l, d); }

    template <bool TEXT>
    Status block_t(const Huff &l, const Huff &d) {
        Bits b = in;
        uint16_t *base = out.data();
        size_t cap = out.size(), m = n;
        Status result = FAIL;
        for (;;) {
            if (m + 600 > cap) {
                if (m + 600 > limit) { result = LIMIT; break; }
                out.resize(std::min(limit, std::max<size_t>(cap * 2, (size_t)1 << 16)));
                base = out.data();
                cap = out.size();
            }
            b.refill();
            Entry e = l.decode(b);
            if (e.op == OP_LIT) {  // the refill covers three codes of 15 bits: most symbols of a text are literals
                if (TEXT && !text_byte(e.val)) break;
                base[m++] = e.val;
                e = l.decode(b);
                if (e.op == OP_LIT) {
                    if (TEXT && !text_byte(e.val)) break;
                    base[m++] = e.val;
                    e = l.decode(b);
                    if (e.op == OP_LIT) {
                        if (TEXT && !text_byte(e.val)) break;
                        base[m++] = e.val;
                        if (b.cnt < 0) break;
                        continue;
                    }
                }
                b.refill();  // (a length + distance needs up to 48 bits)
            }
            if (e.op == OP_EOB) { result = b.cnt < 0 ? FAIL : OK; break; }
            if (e.op < OP_BASE) break;
            const unsigned len = e.val + b.get(e.op - OP_BASE);
            const Entry de = d.decode(b);
            if (de.op < OP_BASE) break;
            const size_t dd = (size_t)de.val + b.get(de.op - OP_BASE);
            if (b.cnt < 0) break;
            uint16_t *o = base + m;
            if (dd <= m) {
                const uint16_t *s = o - dd;
                if (dd >= len) memcpy(o, s, (size_t)len * 2);
                else for (unsigned k = 0; k < len; ++k) o[k] = s[k];
            } else {  // reaches in front of the chunk: markers for the part that does
                const size_t before = dd - m;  // symbols of the match that lie in front of the chunk (if it is that long)
                const unsigned nb = (unsigned)std::min<size_t>(before, len);
                for (unsigned k = 0; k < nb; ++k) o[k] = (uint16_t)(256 + 32768 - before + k);
                for (unsigned k = nb; k < len; ++k) o[k] = base[k - nb];
            }
            m += len;
        }
        in = b;
        n = m;
        return result;
    }

    // the header of a stored block, from behind its three header bits: to the byte boundary, LEN and its complement
    bool stored_header(unsigned *len) {
        in.drop(in.cnt & 7);
        in.refill();
        *len = in.get(16);
        const unsigned nlen = in.get(16);
        return in.cnt >= 0 && (*len ^ nlen) == 0xffffu;
    }

    // one block from its three header bits on; *final_block = BFINAL
    Status any_block(bool *final_block, bool check_text) {
        in.refill();
        if (in.cnt < 3) return FAIL;
        *final_block = in.get(1) != 0;
        const unsigned type = in.get(2);
        if (type == 2) {
            if (!dynamic_header()) return FAIL;
            return block(lit, dist, check_text);
        }
        if (type == 1) {
            ensure_fixed();
            return block(fixed_lit, fixed_dist, check_text);
        }
        if (type != 0) return FAIL;
        unsigned len;
        if (!stored_header(&len)) return FAIL;
        if (n + len + 600 > out.size()) {
            if (n + len + 600 > limit) return LIMIT;
            out.resize(std::min(limit, std::max<size_t>(out.size() * 2, n + len + 600)));
        }
        for (unsigned k = 0; k < len; ++k) {
            if ((k & 3) == 0) in.refill();
            const unsigned c = in.get(8);
            if (check_text && !text_byte(c)) return FAIL;
            out[n++] = (uint16_t)c;
        }
        return in.cnt < 0 ? FAIL : OK;
    }

    // a block header that holds together stands here (what follows a block start that the search accepts)
    bool header_follows() {
        in.refill();
        if (in.cnt < 3) return false;
        in.drop(1);
        const unsigned type = in.get(2);
        unsigned len;
        return type == 2 ? dynamic_header() : type == 0 ? stored_header(&len) : type == 1;
    }
};

// first position in [from, to) that looks like the start of a non-final dynamic block whose content is text and which is followed by
// another well-formed block header
static bool find_block_start(Decoder &probe, uint64_t from, uint64_t to, uint64_t *start) {
    for (uint64_t c = from; c < to; ++c) {
        probe.in.seek(c);
        if (probe.in.cnt < 17) return false;
        const uint32_t h = probe.in.peek(13);
        // BFINAL = 0, BTYPE = 2, HLIT <= 29 (286 length codes), HDIST <= 29
        if ((h & 7) != 4 || ((h >> 3) & 31) > 29 || ((h >> 8) & 31) > 29) continue;
        probe.n = 0;
        bool fin = false;
        if (probe.any_block(&fin, true) != OK || fin || probe.n == 0 || !probe.header_follows()) continue;
        *start = c;
        return true;
    }
    return false;
}

}  // namespace pinflate
