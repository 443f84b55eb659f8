// bam_encode.hip — FASTQ / FASTA record text turned into unaligned BAM records on the GPU: bam.hip the other way round.
//
// the layout pass       (record_pipeline.h) with the Encode codec below: a record's shape is validated (bam_encode.h: text_shape,
//                       the one scan of the header line) and gives its BAM size, its number of emit items and the two lengths
//                       the passes behind need;
// k_bamenc_emit         one workgroup per (record, chunk of ENC_CHUNK bases), grid-stride over the items: a 4 Mbp read is a
//                       thousand items spread over the chip, a 200-base read is one.
// The emit kernel moves ~2 bytes in and 1.5 bytes out per base.  Output positions fall on every alignment, so each of the two parts
// of a chunk (packed bases, qualities) is written as head bytes up to the next 16-byte boundary of the OUTPUT address, whole aligned
// 16-byte stores (one lane each: 32 characters through a 256-entry character -> code table in LDS into 16 packed bytes; 16 quality
// characters checked and lowered by 33 four to a word), and tail bytes.  The table is 256 bytes, one bank row of the LDS: two
// different characters lie in different banks and equal ones broadcast, so the 64 lanes' byte reads never conflict.  Loads take
// exactly the bytes they need at whatever address they lie (the hardware's unaligned global loads): nothing outside a record is
// read, and a record was validated against its own range by the layout pass.  A QUAL byte outside 33..126 is met in the emit pass
// and lowers the call's first bad record like a shape error does in the sizes pass.
#include "flx_internal.h"
#include "bam_encode.h"
#include "record_pipeline.h"

using namespace bamenc;
using recpipe::kStateWords;

namespace {

constexpr int ENC_NT = recpipe::NT;             // threads per workgroup
constexpr uint32_t ENC_CHUNK = recpipe::CHUNK;  // bases per emit item: one 16-byte quality store per lane, one packed store per two

struct Info {  // what the sizes pass found in the header line; l_name == 0: the record's shape is not valid
    uint32_t h, l_name;
};

__device__ __forceinline__ uint64_t items_of(uint64_t l) { return l ? (l + ENC_CHUNK - 1) / ENC_CHUNK : 1; }  // (an empty read still has its fixed part)

// the record text[at, end) again from what the sizes pass kept of it: no second scan of the header line
__device__ __forceinline__ TextRec rebuild(const uint8_t *text, uint64_t at, uint64_t end, Info f) {
    TextRec r;
    r.at = at;
    r.h = f.h;
    r.l_name = f.l_name;
    r.seq = at + f.h + 2;
    r.fasta = text[at] == '>';
    r.l = r.fasta ? end - at - f.h - 3 : (end - at - f.h - 6) / 2;
    r.qual = r.fasta ? end : r.seq + r.l + 3;
    return r;
}

struct Encode {
    using Sums = recpipe::Sum2;
    static size_t extra_bytes(uint64_t n_rec) { return n_rec * sizeof(Info); }
    const uint8_t *text;
    uint64_t n;
    const uint64_t *off;
    Info *info;  // the work block's extra bytes
    __device__ __forceinline__ Sums measure(uint64_t k, bool *bad) const {
        const uint64_t at = off[k], end = off[k + 1];
        TextRec r;
        Info f = {0, 0};
        Sums v = {0, 0};
        *bad = !(at <= end && end <= n && text_shape(text, at, end, r));
        if (!*bad) {
            f = {r.h, r.l_name};
            v = {bam_size(r), items_of(r.l)};
        }
        info[k] = f;
        return v;
    }
    __device__ __forceinline__ Sums recall(uint64_t k) const {
        if (!info[k].l_name) return {0, 0};
        const TextRec r = rebuild(text, off[k], off[k + 1], info[k]);
        return {bam_size(r), items_of(r.l)};
    }
};

// packed byte m of the record through the table
__device__ __forceinline__ uint8_t packed_byte_lut(const uint8_t *text, const TextRec &r, uint64_t m, const uint8_t *lut) {
    const uint32_t hi = lut[text[r.seq + 2 * m]], lo = 2 * m + 1 < r.l ? lut[text[r.seq + 2 * m + 1]] : 0;
    return (uint8_t)(hi << 4 | lo);
}
// four characters as two packed bytes
__device__ __forceinline__ uint32_t pack4(uint32_t w, const uint8_t *lut) {
    return (uint32_t)lut[w & 255] << 4 | (uint32_t)lut[(w >> 8) & 255] | (uint32_t)lut[(w >> 16) & 255] << 12 | (uint32_t)lut[w >> 24] << 8;
}

// The packed bytes [m0, m0 + n) of a record go to dst[0, n); n <= ENC_CHUNK / 2.
__device__ __forceinline__ void emit_packed(const uint8_t *text, const TextRec &r, uint64_t m0, uint32_t n, uint8_t *dst, const uint8_t *lut) {
    const uint32_t t = threadIdx.x;
    auto [head, groups, tail] = recpipe::split16(dst, n);
    // the last byte of an odd L holds one base: it is a tail byte, so that a whole store reads 32 characters of SEQ and no more
    if ((r.l & 1) && m0 + n == (r.l + 1) / 2 && tail == 0 && groups > 0) {
        --groups;
        tail = 16;
    }
    if (t < head) dst[t] = packed_byte_lut(text, r, m0 + t, lut);
    if (t < tail) {
        const uint32_t j = head + 16 * groups + t;
        dst[j] = packed_byte_lut(text, r, m0 + j, lut);
    }
    if (t >= groups) return;  // (groups <= ENC_CHUNK / 32 = ENC_NT / 2)
    const uint64_t m = m0 + head + 16 * (uint64_t)t;  // the group's first packed byte; 2 * (m + 16) <= L
    uint32_t w[8];
    __builtin_memcpy(w, text + r.seq + 2 * m, 32);
    uint4 o;
    o.x = pack4(w[0], lut) | pack4(w[1], lut) << 16;
    o.y = pack4(w[2], lut) | pack4(w[3], lut) << 16;
    o.z = pack4(w[4], lut) | pack4(w[5], lut) << 16;
    o.w = pack4(w[6], lut) | pack4(w[7], lut) << 16;
    *(uint4 *)(dst + head + 16 * (uint64_t)t) = o;
}

// bit 7 of every byte of x that is not in 33..126
__device__ __forceinline__ uint32_t qual_bad4(uint32_t x) {
    const uint32_t lo7 = x & 0x7f7f7f7fu;  // (no sum below carries out of its byte: 127 + 95 < 256)
    return (x | (lo7 + 0x01010101u) | ~(lo7 + 0x5f5f5f5fu)) & 0x80808080u;  // >= 128, == 127, < 33
}

// The quality bytes [j0, j0 + n) of a record go to dst[0, n); n <= ENC_CHUNK.  True when a QUAL byte of this lane was out of range.
__device__ __forceinline__ bool emit_qual(const uint8_t *text, const TextRec &r, uint64_t j0, uint32_t n, uint8_t *dst) {
    const uint32_t t = threadIdx.x;
    const auto [head, groups, tail] = recpipe::split16(dst, n);
    bool bad = false;
    if (t < head) {
        const uint32_t c = r.fasta ? 33 + 0xff : text[r.qual + j0 + t];
        bad = !r.fasta && !qual_byte_ok(c);
        dst[t] = (uint8_t)(c - 33);
    }
    if (t < tail) {
        const uint32_t j = head + 16 * groups + t;
        const uint32_t c = r.fasta ? 33 + 0xff : text[r.qual + j0 + j];
        bad = bad || (!r.fasta && !qual_byte_ok(c));
        dst[j] = (uint8_t)(c - 33);
    }
    if (t >= groups) return bad;  // (groups <= ENC_CHUNK / 16 = ENC_NT: one per lane)
    uint4 o;
    if (r.fasta) {
        o.x = o.y = o.z = o.w = 0xffffffffu;
    } else {
        uint32_t w[4];
        __builtin_memcpy(w, text + r.qual + j0 + head + 16 * (uint64_t)t, 16);
        bad = bad || (qual_bad4(w[0]) | qual_bad4(w[1]) | qual_bad4(w[2]) | qual_bad4(w[3])) != 0;
        // (every byte >= 33: no borrow crosses a byte; with a bad byte the output is no result)
        o.x = w[0] - 0x21212121u; o.y = w[1] - 0x21212121u; o.z = w[2] - 0x21212121u; o.w = w[3] - 0x21212121u;
    }
    *(uint4 *)(dst + head + 16 * (uint64_t)t) = o;
    return bad;
}

__global__ void __launch_bounds__(ENC_NT) k_bamenc_emit(Encode codec, uint64_t n_rec, const uint64_t *out_off, const uint64_t *item_off,
                                                        const uint32_t *item_rec, uint64_t item_cap, unsigned long long *state, uint8_t *out,
                                                        uint64_t out_cap) {
    const uint8_t *text = codec.text;
    const uint64_t *off = codec.off;
    const Info *info = codec.info;
    __shared__ __attribute__((aligned(256))) uint8_t lut[256];
    const uint32_t t = threadIdx.x;
    lut[t] = base_code(t);
    __syncthreads();
    const uint64_t n_items = state[1] < item_cap ? state[1] : item_cap;
    if (state[0] > out_cap) return;  // FLX_ERR_CAPACITY: nothing is written
    for (uint64_t w = blockIdx.x; w < n_items; w += gridDim.x) {
        const uint64_t k = item_rec[w];
        if (k >= n_rec || item_off[k] > w || !info[k].l_name) continue;  // (cannot happen: k_offsets wrote the item)
        const TextRec r = rebuild(text, off[k], off[k + 1], info[k]);
        const uint64_t c = w - item_off[k], o = out_off[k], l = r.l;
        if (c >= items_of(l) || o + bam_size(r) > out_cap) continue;
        uint8_t *name = out + o + 36, *packed = name + r.l_name + 1, *qual = packed + (l + 1) / 2;
        if (c == 0) {  // the record's fixed part and its name
            if (t < 9) {  // nine lanes, one word each (fixed_part: block_size, refID, pos, l_read_name/mapq/bin, n_cigar_op/flag, l_seq, ...)
                const uint32_t word = t == 0 ? (uint32_t)(bam_size(r) - 4) : t == 3 ? (r.l_name + 1) | 4680u << 16 : t == 4 ? 4u << 16 :
                                      t == 5 ? (uint32_t)l : t == 8 ? 0u : 0xffffffffu;
                __builtin_memcpy(out + o + 4 * t, &word, 4);  // (any alignment: an unaligned global store)
            }
            if (t == 9) name[r.l_name] = 0;
            for (uint32_t i = t; i < r.l_name; i += ENC_NT) name[i] = text[r.at + 1 + i];
        }
        const uint64_t b0 = c * ENC_CHUNK;  // (even: a chunk begins with a whole packed byte)
        if (b0 >= l) continue;
        const uint32_t len = (uint32_t)(l - b0 < ENC_CHUNK ? l - b0 : ENC_CHUNK);
        emit_packed(text, r, b0 / 2, (len + 1) / 2, packed + b0 / 2, lut);
        if (emit_qual(text, r, b0, len, qual + b0)) atomicMax(&state[3], (unsigned long long)(n_rec - k));
    }
}

// the most bytes the records of n_text bytes of text can take.  Per record, with T its text length, H >= name >= 1 and L its bases:
//   FASTA  T = H + L + 3, BAM = 37 + name + ceil(L/2) + L:  BAM - T = 34 + name - H + ceil(L/2) <= 34 + ceil(L/2), and L <= T - 4
//          gives ceil(L/2) <= (T - 3) / 2 <= T / 2;
//   FASTQ  T = H + 2L + 6:  BAM - T = 31 + name - H + ceil(L/2) - L <= 31 (L = 0 and L = 1 reach it with H == name).
// So BAM <= T + T / 2 + 34 for either kind, and the sum over the records is at most n_text + n_text / 2 + 34 n_records (the sum of
// the floors is at most the floor of the sum).  A FASTA record of L = 0 with a 1-byte name has T = 4 and BAM = 38 <= 4 + 2 + 34.
uint64_t enc_bound(uint64_t n_text, uint64_t n_records) { return n_text + n_text / 2 + 34 * n_records; }

}  // namespace

size_t flx_bam_encode_work_bytes(uint64_t n_rec, uint64_t bytes) { return recpipe::work_bytes<Encode>(n_rec, bytes); }

unsigned flx_bam_encode_blocks(const flx_ctx *ctx) { return recpipe::emit_blocks_of(ctx); }

// The launches of one call on `st` (n_rec >= 1; `work` has flx_bam_encode_work_bytes(n_rec, n) bytes or more, carved for exactly
// (n_rec, n)): h_state (pinned, or read after a synchronisation) gets [0] the BAM bytes and [3] n_rec - the lowest bad record.
hipError_t flx_bam_encode_launch(hipStream_t st, unsigned emit_blocks, const void *d_text, uint64_t n, const uint64_t *d_off, uint64_t n_rec,
                                 void *work, uint64_t *d_out_off, void *d_out, uint64_t out_cap, uint64_t *h_state) {
    const auto w = recpipe::carve<Encode>(work, n_rec, n);
    return recpipe::launch(st, emit_blocks, Encode{(const uint8_t *)d_text, n, d_off, (Info *)w.extra}, n_rec, w, d_out_off, k_bamenc_emit, d_out,
                           out_cap, h_state);
}

extern "C" int flx_bam_header(void *out, uint64_t out_cap, uint64_t *out_len) {
    if (!out_len) return FLX_ERR_INVALID;
    *out_len = kHeaderLen;
    if (!out) return FLX_OK;
    if (out_cap < kHeaderLen) return FLX_ERR_CAPACITY;
    write_header((uint8_t *)out);
    return FLX_OK;
}

extern "C" int flx_bam_from_fastq_bound(uint64_t n_text, uint64_t n_records, uint64_t *bound) {
    if (!bound) return FLX_ERR_INVALID;
    *bound = enc_bound(n_text, n_records);
    return FLX_OK;
}

extern "C" int flx_bam_from_fastq_dev(flx_ctx *ctx, const void *d_text, uint64_t n, const uint64_t *d_rec_off, uint64_t n_records, void *d_out,
                                      uint64_t out_cap, uint64_t *d_out_off, uint64_t *out_len, uint64_t *first_bad) {
    if (!ctx) return FLX_ERR_INVALID;
    if (!out_len || !first_bad) return flx_fail(ctx, FLX_ERR_INVALID, "flx_bam_from_fastq_dev: bad argument");
    *out_len = 0;
    *first_bad = n_records;
    if (n_records == 0) return FLX_OK;
    if (!d_text || !d_rec_off || !d_out_off || (!d_out && out_cap) || n_records > 0xffffffffull)
        return flx_fail(ctx, FLX_ERR_INVALID, "flx_bam_from_fastq_dev: bad argument");
    void *work = nullptr;
    FLX_CHECK(flx_scratch(ctx, flx_bam_encode_work_bytes(n_records, n), &work));
    uint64_t st[kStateWords] = {0, 0, 0, 0};
    flx_time_scope ts(ctx, "flx_bam_encode");
    hipError_t e = flx_bam_encode_launch(ctx->stream, flx_bam_encode_blocks(ctx), d_text, n, d_rec_off, n_records, work, d_out_off, d_out, out_cap, st);
    ts.end();
    return recpipe::finish_dev(ctx, "flx_bam_from_fastq_dev", e, st, n_records, out_cap, out_len, first_bad);
}
