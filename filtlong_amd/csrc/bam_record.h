// bam_record.h — BAM records to FASTQ text: the record core of bam.hip, shared by the kernels and the host walk.
//
// Like bgzf_inflate_member.h: plain C++ that a HIP kernel and a host program both include.  The layout is restated from the
// SAM/BAM specification, section 4.2 (all integers little-endian):
//   header   magic "BAM\1", i32 l_text, the text, i32 n_ref, then per reference i32 l_name, the name, i32 l_ref;
//   record   u32 block_size, then block_size bytes: i32 refID, i32 pos, u8 l_read_name, u8 mapq, u16 bin, u16 n_cigar_op, u16 flag,
//            i32 l_seq, i32 next_refID, i32 next_pos, i32 tlen (32 bytes), the name (l_read_name bytes, NUL-terminated),
//            the CIGAR (4 * n_cigar_op bytes), the bases (4 bits each, high nibble first, (l_seq + 1) / 2 bytes), the qualities
//            (l_seq bytes), the tags (the rest).  CIGAR and tags are skipped, never interpreted.
// A record is valid when block_size >= 32, l_read_name >= 1, l_seq >= 0, the five parts fit block_size, the record lies inside
// the buffer and the name's last byte is NUL; every sum is carried in 64 bits.
//
// The text of a record is '@' name '\n' SEQ '\n' '+' '\n' QUAL '\n' (l_read_name + 2 * l_seq + 5 bytes):
//   SEQ    "=ACMGRSVTWYHKDBN"[code];
//   QUAL   min(q, 93) + 33; when the FIRST quality byte is 0xFF no qualities are stored and every position is '"' (quality 1);
//   flag 0x10            SEQ reverse-complemented (IUPAC: the complement of a 4-bit code is its bits in reverse order, so '=' and
//                        'N' stay) and QUAL reversed;
//   flag 0x100 / 0x800   (secondary, supplementary) and l_seq == 0: no text, the record is skipped and counted;
//   flags 0x40 / 0x80    do not change the name.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define BAM_FN __host__ __device__ __forceinline__
#else
#define BAM_FN inline
#endif

namespace bam {

enum RecStatus : int {
    REC_OK = 0,
    REC_END = 1,        // no byte left: the records end here
    REC_TRUNCATED = 2,  // the data ends inside the record
    REC_BAD = 3         // a field breaks a rule above
};

constexpr uint32_t FLAG_REVERSE = 0x10, FLAG_NO_TEXT = 0x100 | 0x800;

struct Rec {
    uint64_t name, seq, qual;  // offsets of the parts in the buffer
    uint64_t end;              // offset of the next record
    uint32_t l_name, flag;
    int32_t l_seq;
};

BAM_FN uint32_t rd16(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }
BAM_FN uint32_t rd32(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }

// the record at `at` of buf[0, n); reads no byte outside [at, n)
BAM_FN int read_record(const uint8_t *buf, uint64_t n, uint64_t at, Rec &r) {
    if (at >= n) return REC_END;
    if (n - at < 4) return REC_TRUNCATED;
    const uint64_t block_size = rd32(buf + at);
    if (block_size < 32) return REC_BAD;
    if (n - at - 4 < 32) return REC_TRUNCATED;
    const uint8_t *f = buf + at + 4;
    const uint64_t l_name = f[8], n_cigar = rd16(f + 12);
    const int32_t l_seq = (int32_t)rd32(f + 16);
    if (l_name < 1 || l_seq < 0) return REC_BAD;
    const uint64_t l = (uint64_t)l_seq;
    if (32 + l_name + 4 * n_cigar + (l + 1) / 2 + l > block_size) return REC_BAD;
    if (n - at - 4 < block_size) return REC_TRUNCATED;
    r.name = at + 36;
    if (buf[r.name + l_name - 1] != 0) return REC_BAD;
    r.seq = r.name + l_name + 4 * n_cigar;
    r.qual = r.seq + (l + 1) / 2;
    r.end = at + 4 + block_size;
    r.l_name = (uint32_t)l_name;
    r.flag = rd16(f + 14);
    r.l_seq = l_seq;
    return REC_OK;
}

BAM_FN bool has_text(const Rec &r) { return !(r.flag & FLAG_NO_TEXT) && r.l_seq > 0; }
BAM_FN uint64_t text_size(const Rec &r) { return has_text(r) ? (uint64_t)r.l_name + 2 * (uint64_t)r.l_seq + 5 : 0; }

// The header of buf[0, n): REC_OK and *end = the offset of the first record, REC_TRUNCATED when the data ends inside it, else REC_BAD.
BAM_FN int read_header(const uint8_t *buf, uint64_t n, uint64_t *end) {
    const uint8_t magic[4] = {'B', 'A', 'M', 1};
    for (uint64_t i = 0; i < 4; ++i) {
        if (i >= n) return REC_TRUNCATED;
        if (buf[i] != magic[i]) return REC_BAD;
    }
    uint64_t at = 4;
    if (n - at < 4) return REC_TRUNCATED;
    const int32_t l_text = (int32_t)rd32(buf + at);
    at += 4;
    if (l_text < 0) return REC_BAD;
    if (n - at < (uint64_t)l_text) return REC_TRUNCATED;
    at += (uint64_t)l_text;
    if (n - at < 4) return REC_TRUNCATED;
    const int32_t n_ref = (int32_t)rd32(buf + at);
    at += 4;
    if (n_ref < 0) return REC_BAD;
    for (int32_t k = 0; k < n_ref; ++k) {
        if (n - at < 4) return REC_TRUNCATED;
        const int32_t l_name = (int32_t)rd32(buf + at);
        at += 4;
        if (l_name < 0) return REC_BAD;
        if (n - at < (uint64_t)l_name) return REC_TRUNCATED;
        at += (uint64_t)l_name;
        if (n - at < 4) return REC_TRUNCATED;
        at += 4;
    }
    *end = at;
    return REC_OK;
}

// ---- the characters of a record's text ---------------------------------------------------------------------------------------
BAM_FN uint32_t complement_code(uint32_t c) { return (c & 1) << 3 | (c & 2) << 1 | (c & 4) >> 1 | (c & 8) >> 3; }
BAM_FN uint8_t code_char(uint32_t c) {  // "=ACMGRSVTWYHKDBN"[c]
    const uint64_t lo = 0x565352474d43413dull, hi = 0x4e42444b48595754ull;
    return (uint8_t)((c < 8 ? lo : hi) >> (8 * (c & 7)));
}
BAM_FN uint8_t qual_char(uint32_t q) { return (uint8_t)((q < 93 ? q : 93) + 33); }
constexpr uint8_t kMissingQual = '"';  // quality 1

// character j of the SEQ line / of the QUAL line, 0 <= j < l_seq
BAM_FN uint8_t seq_char_at(const uint8_t *buf, const Rec &r, uint64_t j) {
    const bool rev = r.flag & FLAG_REVERSE;
    const uint64_t i = rev ? (uint64_t)r.l_seq - 1 - j : j;
    const uint32_t b = buf[r.seq + (i >> 1)], c = (i & 1) ? (b & 15) : (b >> 4);
    return code_char(rev ? complement_code(c) : c);
}
BAM_FN uint8_t qual_char_at(const uint8_t *buf, const Rec &r, uint64_t j) {
    if (buf[r.qual] == 0xff) return kMissingQual;
    return qual_char(buf[r.qual + ((r.flag & FLAG_REVERSE) ? (uint64_t)r.l_seq - 1 - j : j)]);
}

// the two characters of a packed byte: forward (high nibble first) and reverse-complemented (low nibble first)
BAM_FN uint16_t pair_chars(uint32_t b, bool rev) {
    const uint32_t first = rev ? complement_code(b & 15) : (b >> 4), second = rev ? complement_code(b >> 4) : (b & 15);
    return (uint16_t)(code_char(first) | (uint32_t)code_char(second) << 8);
}

// ---- the host walk -------------------------------------------------------------------------------------------------------
// the text of a record that has one, text_size(r) bytes at `out`
inline void emit_record_host(const uint8_t *buf, const Rec &r, uint8_t *out) {
    static const struct Tables {
        uint16_t fwd[256];
        Tables() {
            for (uint32_t b = 0; b < 256; ++b) fwd[b] = pair_chars(b, false);
        }
    } T;
    const uint64_t l = (uint64_t)r.l_seq;
    const bool rev = r.flag & FLAG_REVERSE;
    uint8_t *o = out;
    *o++ = '@';
    for (uint32_t i = 0; i + 1 < r.l_name; ++i) *o++ = buf[r.name + i];
    *o++ = '\n';
    const uint8_t *s = buf + r.seq, *q = buf + r.qual;
    if (!rev) {
        for (uint64_t m = 0; m < l / 2; ++m) {
            const uint16_t two = T.fwd[s[m]];
            o[2 * m] = (uint8_t)two;
            o[2 * m + 1] = (uint8_t)(two >> 8);
        }
        if (l & 1) o[l - 1] = (uint8_t)T.fwd[s[l / 2]];
    } else {
        for (uint64_t j = 0; j < l; ++j) o[j] = seq_char_at(buf, r, j);
    }
    o += l;
    *o++ = '\n';
    *o++ = '+';
    *o++ = '\n';
    if (q[0] == 0xff) {
        for (uint64_t j = 0; j < l; ++j) o[j] = kMissingQual;
    } else if (!rev) {
        for (uint64_t j = 0; j < l; ++j) o[j] = qual_char(q[j]);
    } else {
        for (uint64_t j = 0; j < l; ++j) o[j] = qual_char(q[l - 1 - j]);
    }
    o += l;
    *o = '\n';
}

enum EndState : int {
    END_OF_DATA = 0,   // the last record ends where the data ends
    END_TRUNCATED = 1, // the data ends inside the header or inside record *n_records
    END_MALFORMED = 2, // record *n_records breaks a rule
    END_HEADER = 3,    // the header does: no magic, a negative length
    END_MORE = 4       // max_records were taken and data is left
};

// The records of buf[0, n): rec_off[0..m] (when not null; room for max_records + 1) and the count; the end state as above.
inline int index_host(const uint8_t *buf, uint64_t n, uint64_t max_records, uint64_t *rec_off, uint64_t *n_records) {
    uint64_t at = 0, m = 0;
    *n_records = 0;
    if (rec_off) rec_off[0] = 0;
    const int h = read_header(buf, n, &at);
    if (h != REC_OK) return h == REC_TRUNCATED ? END_TRUNCATED : END_HEADER;
    if (rec_off) rec_off[0] = at;
    int end = END_MORE;
    while (m < max_records) {
        Rec r;
        const int st = read_record(buf, n, at, r);
        if (st != REC_OK) {
            end = st == REC_END ? END_OF_DATA : st == REC_TRUNCATED ? END_TRUNCATED : END_MALFORMED;
            break;
        }
        at = r.end;
        ++m;
        if (rec_off) rec_off[m] = at;
    }
    if (end == END_MORE && at >= n) end = END_OF_DATA;
    *n_records = m;
    return end;
}

// Records [k0, k1) of an index: their text sizes summed, and the count of those without text.  The records were valid for
// index_host, so read_record cannot fail.
inline uint64_t text_bytes_host(const uint8_t *buf, const uint64_t *rec_off, uint64_t k0, uint64_t k1, uint64_t *n_skipped) {
    uint64_t bytes = 0, skipped = 0;
    for (uint64_t k = k0; k < k1; ++k) {
        Rec r;
        if (read_record(buf, rec_off[k + 1], rec_off[k], r) != REC_OK) continue;
        bytes += text_size(r);
        skipped += !has_text(r);
    }
    if (n_skipped) *n_skipped = skipped;
    return bytes;
}

// the text of records [k0, k1) at `out` (text_bytes_host(...) bytes)
inline void emit_records_host(const uint8_t *buf, const uint64_t *rec_off, uint64_t k0, uint64_t k1, uint8_t *out) {
    for (uint64_t k = k0; k < k1; ++k) {
        Rec r;
        if (read_record(buf, rec_off[k + 1], rec_off[k], r) != REC_OK || !has_text(r)) continue;
        emit_record_host(buf, r, out);
        out += text_size(r);
    }
}
}  // namespace bam
