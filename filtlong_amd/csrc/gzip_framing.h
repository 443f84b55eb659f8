// gzip_framing.h — where a gzip member begins and ends (RFC 1952), and which members are BGZF blocks (SAM specification 4.1).
// Host only, nothing but the bytes: flx_bgzf_index (bgzf_inflate.hip) and the command line's readers (cli/inflate_stream.h,
// cli/pinflate_rounds.h) all take a member for what this file says it is.  No function reads a byte at or behind `size`.
#pragma once
#include <cstddef>
#include <cstdint>

namespace gzframe {

inline uint32_t le16(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }
inline uint32_t le32(const uint8_t *p) { return le16(p) | le16(p + 2) << 16; }

// "a member follows": the two magic bytes at `at` (all that gzread looks at between members)
inline bool magic_at(const uint8_t *d, size_t size, size_t at) { return at + 2 <= size && d[at] == 0x1f && d[at + 1] == 0x8b; }

struct Header {
    size_t deflate_at = 0;  // the first byte of the deflate data
    size_t bgzf_size = 0;   // BSIZE + 1 of a `BC` subfield with SLEN 2 that lies inside the extra field (the last, if several); 0: none
};

// The header of a member at `at`: at least 26 bytes from there, magic, CM = 8, no reserved flag bit; FEXTRA, FNAME, FCOMMENT and
// FHCRC are skipped; more than the 8 bytes of a trailer are left behind it.
inline bool parse_header(const uint8_t *d, size_t size, size_t at, Header *h) {
    *h = Header();
    if (at + 18 + 8 > size || !magic_at(d, size, at) || d[at + 2] != 8) return false;
    const unsigned flg = d[at + 3];
    if (flg & 0xe0) return false;
    size_t p = at + 10;
    if (flg & 4) {
        const size_t xlen = le16(d + p);
        p += 2;
        if (p + xlen > size) return false;
        for (size_t q = p; q + 4 <= p + xlen;) {
            const size_t slen = le16(d + q + 2);
            if (d[q] == 'B' && d[q + 1] == 'C' && slen == 2 && q + 6 <= p + xlen) h->bgzf_size = (size_t)le16(d + q + 4) + 1;
            q += 4 + slen;
        }
        p += xlen;
    }
    for (unsigned f = 8; f <= 16; f <<= 1)  // FNAME, FCOMMENT: zero-terminated
        if (flg & f) {
            while (p < size && d[p]) ++p;
            ++p;
        }
    if (flg & 2) p += 2;
    if (p + 8 >= size) return false;
    h->deflate_at = p;
    return true;
}

// What stands at `at`.  A BGZF block names its own size, ends inside the data, has room for its header and trailer, and claims
// at most 64 KiB of output; one that claims more is no BGZF block or a damaged one (FORGED: zlib's, from that byte).
enum class Kind { NONE /* no magic: the end */, OTHER /* a member (or a damaged header) that is not BGZF */, BGZF, FORGED };
struct Member {
    size_t size = 0;     // BGZF, FORGED: the whole member, header to trailer
    uint32_t isize = 0;  // ... and the trailer's ISIZE
};
inline Kind member_at(const uint8_t *d, size_t size, size_t at, Member *m) {
    *m = Member();
    if (!magic_at(d, size, at)) return Kind::NONE;
    Header h;
    if (!parse_header(d, size, at, &h) || h.bgzf_size == 0 || at + h.bgzf_size > size || h.bgzf_size < h.deflate_at - at + 8)
        return Kind::OTHER;
    m->size = h.bgzf_size;
    m->isize = le32(d + at + h.bgzf_size - 4);
    return m->isize > 65536 ? Kind::FORGED : Kind::BGZF;
}

// The end of a member whose deflate data ended in front of byte `at`, for a reader that has the CRC-32 and the length of what it
// decoded: the trailer is cut off (to gzread the end of the file, no error), does not match, or matches — then the member is the
// last, or another follows at *next.
enum class End { TRUNCATED, MISMATCH, LAST, MEMBER_FOLLOWS };
inline End member_end(const uint8_t *d, size_t size, size_t at, uint32_t crc, uint32_t isize, size_t *next) {
    if (at + 8 > size) return End::TRUNCATED;
    if (le32(d + at) != crc || le32(d + at + 4) != isize) return End::MISMATCH;
    *next = at + 8;
    return magic_at(d, size, *next) ? End::MEMBER_FOLLOWS : End::LAST;
}

}  // namespace gzframe
