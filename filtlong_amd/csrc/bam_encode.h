// bam_encode.h — FASTQ / FASTA record text to unaligned BAM records: the record core of bam_encode.hip, shared by the kernels and
// the host walk.  The inverse of bam_record.h, and like it plain C++ that a HIP kernel and a host program both include.
//
// Input is STRICT record text, the form the command line's Emitter writes.  Record k is the bytes [rec_off[k], rec_off[k+1]):
//   '@' HEADER '\n' SEQ '\n' '+' '\n' QUAL '\n'      FASTQ, |SEQ| == |QUAL| == L:  len = H + 2L + 6 (the remainder must be even)
//   '>' HEADER '\n' SEQ '\n'                          FASTA:                        len = H + L + 3
// Only the header line is scanned, up to its first '\n'; L follows from the record's length, and the bytes at the derived positions
// must be '\n', '+', '\n' and '\n'.  The name is the header up to its first blank or tab; the rest of the line is not stored.
// A record is valid when it has that shape, the name has 1..254 bytes, L <= 2^31 - 1 and every QUAL byte is in 33..126 (the
// last rule is the only one that reads the record's body: text_shape checks the others, qual_ok that one).
//
// The BAM record of a valid text record (SAM/BAM specification 4.2, the layout at the top of bam_record.h):
//   block_size, refID -1, pos -1, l_read_name = name + 1, mapq 0, bin 4680, n_cigar_op 0, flag 4, l_seq L, next_refID -1,
//   next_pos -1, tlen 0, the name and a NUL, (L + 1) / 2 packed bytes (high nibble first, a zero low nibble behind an odd L),
//   L quality bytes c - 33 (0xFF at every position for a FASTA record), no tags:  37 + name + (L + 1) / 2 + L bytes.
// A base code is the index of the upper-cased character in "=ACMGRSVTWYHKDBN", 15 ('N') for any other byte: SEQ is mapped, never
// judged.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define BAMENC_FN __host__ __device__ __forceinline__
#else
#define BAMENC_FN inline
#endif

namespace bamenc {

struct TextRec {
    uint64_t at;      // offset of the record's first byte ('@' or '>')
    uint64_t seq;     // offset of SEQ
    uint64_t qual;    // offset of QUAL (FASTQ)
    uint64_t l;       // L
    uint32_t h;       // bytes of the header line between the mark and its '\n'
    uint32_t l_name;  // bytes of the name (without the NUL)
    bool fasta;
};

// the header of a file written from text
constexpr uint32_t kHeaderTextLen = 22;
constexpr uint32_t kHeaderLen = 4 + 4 + kHeaderTextLen + 4;
inline void write_header(uint8_t *out) {
    const char text[kHeaderTextLen + 1] = "@HD\tVN:1.6\tSO:unknown\n";
    out[0] = 'B'; out[1] = 'A'; out[2] = 'M'; out[3] = 1;
    out[4] = kHeaderTextLen; out[5] = out[6] = out[7] = 0;
    for (uint32_t i = 0; i < kHeaderTextLen; ++i) out[8 + i] = (uint8_t)text[i];
    for (uint32_t i = 0; i < 4; ++i) out[8 + kHeaderTextLen + i] = 0;
}

// the code of a SEQ character
BAMENC_FN uint8_t base_code(uint32_t c) {
    if (c >= 'a' && c <= 'z') c -= 32;
    switch (c) {
        case '=': return 0;
        case 'A': return 1;
        case 'C': return 2;
        case 'M': return 3;
        case 'G': return 4;
        case 'R': return 5;
        case 'S': return 6;
        case 'V': return 7;
        case 'T': return 8;
        case 'W': return 9;
        case 'Y': return 10;
        case 'H': return 11;
        case 'K': return 12;
        case 'D': return 13;
        case 'B': return 14;
        default: return 15;
    }
}

// The shape of the record text[at, end) (every rule but the QUAL bytes'); reads no byte outside [at, end).
BAMENC_FN bool text_shape(const uint8_t *text, uint64_t at, uint64_t end, TextRec &r) {
    if (end < at || end - at < 3) return false;
    const uint64_t len = end - at;
    const uint8_t mark = text[at];
    if (mark != '@' && mark != '>') return false;
    uint64_t i = at + 1, name_end = 0;
    bool in_name = true;
    for (; i < end && text[i] != '\n'; ++i)
        if (in_name && (text[i] == ' ' || text[i] == '\t')) {
            in_name = false;
            name_end = i;
        }
    if (i >= end) return false;  // a header line without an end
    if (in_name) name_end = i;
    const uint64_t h = i - (at + 1), l_name = name_end - (at + 1);
    if (l_name < 1 || l_name > 254 || h > 0xffffffffull) return false;
    r.at = at;
    r.h = (uint32_t)h;
    r.l_name = (uint32_t)l_name;
    r.seq = at + h + 2;
    r.fasta = mark == '>';
    if (r.fasta) {
        if (len < h + 3) return false;
        r.l = len - h - 3;
        r.qual = end;
    } else {
        if (len < h + 6 || ((len - h - 6) & 1)) return false;
        r.l = (len - h - 6) / 2;
        r.qual = r.seq + r.l + 3;
        if (text[r.seq + r.l] != '\n' || text[r.seq + r.l + 1] != '+' || text[r.seq + r.l + 2] != '\n') return false;
    }
    if (r.l > 0x7fffffffull || text[end - 1] != '\n') return false;
    return true;
}

BAMENC_FN uint64_t bam_size(const TextRec &r) { return 37 + (uint64_t)r.l_name + (r.l + 1) / 2 + r.l; }
BAMENC_FN bool qual_byte_ok(uint32_t c) { return c >= 33 && c <= 126; }

// the 36 bytes in front of the name
BAMENC_FN void fixed_part(const TextRec &r, uint8_t *f) {
    const uint32_t block_size = (uint32_t)(bam_size(r) - 4), l_seq = (uint32_t)r.l;
    for (int i = 0; i < 36; ++i) f[i] = 0;
    for (int i = 0; i < 4; ++i) {
        f[i] = (uint8_t)(block_size >> (8 * i));
        f[4 + i] = f[8 + i] = 0xff;   // refID, pos
        f[20 + i] = (uint8_t)(l_seq >> (8 * i));
        f[24 + i] = f[28 + i] = 0xff;  // next_refID, next_pos
    }
    f[12] = (uint8_t)(r.l_name + 1);
    f[14] = 4680 & 255;  // bin
    f[15] = 4680 >> 8;
    f[18] = 4;  // flag: unmapped
}

// packed byte m of the record's bases, 0 <= m < (L + 1) / 2
BAMENC_FN uint8_t packed_byte_at(const uint8_t *text, const TextRec &r, uint64_t m) {
    const uint32_t hi = base_code(text[r.seq + 2 * m]), lo = 2 * m + 1 < r.l ? base_code(text[r.seq + 2 * m + 1]) : 0;
    return (uint8_t)(hi << 4 | lo);
}

// ---- the host walk -------------------------------------------------------------------------------------------------------
// the record of a valid text at `out` (bam_size(r) bytes)
inline void emit_record_host(const uint8_t *text, const TextRec &r, uint8_t *out) {
    fixed_part(r, out);
    uint8_t *o = out + 36;
    for (uint32_t i = 0; i < r.l_name; ++i) *o++ = text[r.at + 1 + i];
    *o++ = 0;
    for (uint64_t m = 0; m < (r.l + 1) / 2; ++m) *o++ = packed_byte_at(text, r, m);
    for (uint64_t j = 0; j < r.l; ++j) *o++ = r.fasta ? 0xff : (uint8_t)(text[r.qual + j] - 33);
}

// the QUAL bytes of a record of valid shape
inline bool qual_ok_host(const uint8_t *text, const TextRec &r) {
    if (!r.fasta)
        for (uint64_t j = 0; j < r.l; ++j)
            if (!qual_byte_ok(text[r.qual + j])) return false;
    return true;
}
inline bool shape_host(const uint8_t *text, uint64_t n, uint64_t at, uint64_t end, TextRec &r) {
    return at <= end && end <= n && text_shape(text, at, end, r);
}

// Records [0, n_records) of text[0, n): out_off[0..n_records] (when not null) and the return value are the offsets and the sum of
// the BAM sizes; *first_bad = the lowest invalid record, or n_records.  As in the kernels, a record of invalid shape counts as no
// bytes and one whose only fault is a QUAL byte keeps its size: with an invalid record the output is no result either way.
inline uint64_t sizes_host(const uint8_t *text, uint64_t n, const uint64_t *rec_off, uint64_t n_records, uint64_t *out_off, uint64_t *first_bad) {
    uint64_t bytes = 0, bad = n_records;
    if (out_off) out_off[0] = 0;
    for (uint64_t k = 0; k < n_records; ++k) {
        TextRec r;
        const bool shape = shape_host(text, n, rec_off[k], rec_off[k + 1], r);
        if (shape) bytes += bam_size(r);
        if (bad == n_records && !(shape && qual_ok_host(text, r))) bad = k;
        if (out_off) out_off[k + 1] = bytes;
    }
    if (first_bad) *first_bad = bad;
    return bytes;
}

// the BAM records of records [0, n_records) at `out` (sizes_host(...) bytes)
inline void emit_records_host(const uint8_t *text, uint64_t n, const uint64_t *rec_off, uint64_t n_records, uint8_t *out) {
    for (uint64_t k = 0; k < n_records; ++k) {
        TextRec r;
        if (!shape_host(text, n, rec_off[k], rec_off[k + 1], r)) continue;
        emit_record_host(text, r, out);
        out += bam_size(r);
    }
}
}  // namespace bamenc
