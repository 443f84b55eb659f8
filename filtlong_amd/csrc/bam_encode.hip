// bam_encode.hip — FASTQ / FASTA record text turned into unaligned BAM records on the GPU: bam.hip the other way round, with the
// same four launches.
//
// k_bamenc_sizes        one thread per record: validates its shape (bam_encode.h: text_shape, the one scan of the header line) and
//                       gives its BAM size, its number of emit items and the two lengths the emit pass needs; the tile's sums;
// k_bamenc_scan_tiles   one workgroup: exclusive scan of the tiles' sums and the totals;
// k_bamenc_offsets      the scan inside each tile: out_off[k], item_off[k], and the record of every emit item;
// k_bamenc_emit         one workgroup per (record, chunk of ENC_CHUNK bases), grid-stride over the items: a 4 Mbp read is a
//                       thousand items spread over the chip, a 200-base read is one.
// The emit kernel moves ~2 bytes in and 1.5 bytes out per base.  Output positions fall on every alignment, so each of the two parts
// of a chunk (packed bases, qualities) is written as head bytes up to the next 16-byte boundary of the OUTPUT address, whole aligned
// 16-byte stores (one lane each: 32 characters through a 256-entry character -> code table in LDS into 16 packed bytes; 16 quality
// characters checked and lowered by 33 four to a word), and tail bytes.  The table is 256 bytes, one bank row of the LDS: two
// different characters lie in different banks and equal ones broadcast, so the 64 lanes' byte reads never conflict.  Loads take
// exactly the bytes they need at whatever address they lie (the hardware's unaligned global loads): nothing outside a record is
// read, and a record was validated against its own range by k_bamenc_sizes.  A QUAL byte outside 33..126 is met in the emit pass
// and lowers the call's first bad record like a shape error does in the sizes pass.
#include "flx_internal.h"
#include "bam_encode.h"

using namespace bamenc;

namespace {

constexpr int ENC_NT = 256;                    // threads per workgroup, records per tile
constexpr uint32_t ENC_CHUNK = 16 * ENC_NT;    // bases per emit item: one 16-byte quality store per lane, one packed store per two
constexpr unsigned kEmitBlocksPerCU = 8;

struct Sum2 {
    unsigned long long bytes, items;
};
struct Info {  // what the sizes pass found in the header line; l_name == 0: the record's shape is not valid
    uint32_t h, l_name;
};
// the call's state on the device (zeroed before the launches): [0] BAM bytes, [1] emit items, [2] unused,
// [3] n_records - the lowest bad record (0: none; an atomicMax over the bad records)
constexpr int kStateWords = 4;

__device__ __forceinline__ Sum2 add2(Sum2 a, Sum2 b) { return {a.bytes + b.bytes, a.items + b.items}; }

// exclusive scan of one value per thread over the workgroup; *total gets the sum (every thread)
__device__ __forceinline__ Sum2 block_excl_scan2(Sum2 v, Sum2 *total) {
    __shared__ Sum2 buf[2][ENC_NT];
    const int t = threadIdx.x;
    int cur = 0;
    buf[0][t] = v;
    __syncthreads();
    for (int d = 1; d < ENC_NT; d <<= 1) {
        Sum2 x = buf[cur][t];
        if (t >= d) x = add2(x, buf[cur][t - d]);
        buf[cur ^ 1][t] = x;
        cur ^= 1;
        __syncthreads();
    }
    const Sum2 incl = buf[cur][t];
    *total = buf[cur][ENC_NT - 1];
    __syncthreads();  // (the next call writes buf[0])
    return {incl.bytes - v.bytes, incl.items - v.items};
}

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

__global__ void __launch_bounds__(ENC_NT) k_bamenc_sizes(const uint8_t *text, uint64_t n, const uint64_t *off, uint64_t n_rec, Info *info,
                                                         Sum2 *tile_sums, unsigned long long *state) {
    const uint64_t k = (uint64_t)blockIdx.x * ENC_NT + threadIdx.x;
    Sum2 v = {0, 0};
    if (k < n_rec) {
        const uint64_t at = off[k], end = off[k + 1];
        TextRec r;
        Info f = {0, 0};
        if (at <= end && end <= n && text_shape(text, at, end, r)) {
            f = {r.h, r.l_name};
            v = {bam_size(r), items_of(r.l)};
        } else {
            atomicMax(&state[3], (unsigned long long)(n_rec - k));
        }
        info[k] = f;
    }
    Sum2 total;
    block_excl_scan2(v, &total);
    if (threadIdx.x == 0) tile_sums[blockIdx.x] = total;
}

__global__ void __launch_bounds__(ENC_NT) k_bamenc_scan_tiles(Sum2 *tile_sums, uint64_t n_tiles, unsigned long long *state) {
    Sum2 carry = {0, 0};
    for (uint64_t base = 0; base < n_tiles; base += ENC_NT) {
        const uint64_t i = base + threadIdx.x;
        const Sum2 v = i < n_tiles ? tile_sums[i] : Sum2{0, 0};
        Sum2 total;
        const Sum2 ex = block_excl_scan2(v, &total);
        if (i < n_tiles) tile_sums[i] = add2(carry, ex);
        carry = add2(carry, total);
    }
    if (threadIdx.x == 0) {
        state[0] = carry.bytes;
        state[1] = carry.items;
    }
}

__global__ void __launch_bounds__(ENC_NT) k_bamenc_offsets(const uint8_t *text, const uint64_t *off, uint64_t n_rec, const Info *info,
                                                           const Sum2 *tile_sums, const unsigned long long *state, uint64_t *out_off,
                                                           uint64_t *item_off, uint32_t *item_rec, uint64_t item_cap) {
    const uint64_t k = (uint64_t)blockIdx.x * ENC_NT + threadIdx.x;
    Sum2 v = {0, 0};
    if (k < n_rec && info[k].l_name) {
        const TextRec r = rebuild(text, off[k], off[k + 1], info[k]);
        v = {bam_size(r), items_of(r.l)};
    }
    Sum2 total;
    const Sum2 ex = add2(tile_sums[blockIdx.x], block_excl_scan2(v, &total));
    if (k >= n_rec) return;
    out_off[k] = ex.bytes;
    item_off[k] = ex.items;
    if (k == n_rec - 1) {
        out_off[n_rec] = state[0];
        item_off[n_rec] = state[1];
    }
    // (item_cap is the host's bound of the item count, n_rec + bytes / ENC_CHUNK: records whose ranges do not overlap cannot
    // exceed it, and the test keeps any others from writing outside the array)
    for (uint64_t c = 0; c < v.items && ex.items + c < item_cap; ++c) item_rec[ex.items + c] = (uint32_t)k;
}

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
    uint32_t head = (uint32_t)(-(uintptr_t)dst & 15);
    if (head > n) head = n;
    uint32_t groups = (n - head) / 16, tail = n - head - 16 * groups;
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
    uint32_t head = (uint32_t)(-(uintptr_t)dst & 15);
    if (head > n) head = n;
    const uint32_t groups = (n - head) / 16, tail = n - head - 16 * groups;
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

__global__ void __launch_bounds__(ENC_NT) k_bamenc_emit(const uint8_t *text, const uint64_t *off, uint64_t n_rec, const Info *info,
                                                        const uint64_t *out_off, const uint64_t *item_off, const uint32_t *item_rec,
                                                        uint64_t item_cap, unsigned long long *state, uint8_t *out, uint64_t out_cap) {
    __shared__ __attribute__((aligned(256))) uint8_t lut[256];
    const uint32_t t = threadIdx.x;
    lut[t] = base_code(t);
    __syncthreads();
    const uint64_t n_items = state[1] < item_cap ? state[1] : item_cap;
    if (state[0] > out_cap) return;  // FLX_ERR_CAPACITY: nothing is written
    for (uint64_t w = blockIdx.x; w < n_items; w += gridDim.x) {
        const uint64_t k = item_rec[w];
        if (k >= n_rec || item_off[k] > w || !info[k].l_name) continue;  // (cannot happen: k_bamenc_offsets wrote the item)
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

uint64_t item_bound(uint64_t n_rec, uint64_t bytes) { return n_rec + bytes / ENC_CHUNK; }
uint64_t n_tiles_of(uint64_t n_rec) { return (n_rec + ENC_NT - 1) / ENC_NT; }

struct EncWork {  // the device arrays of one call, carved out of one block
    Sum2 *tile_sums;
    unsigned long long *state;
    uint64_t *item_off;
    Info *info;
    uint32_t *item_rec;
    uint64_t item_cap;
};
EncWork carve(void *p, uint64_t n_rec, uint64_t bytes) {
    EncWork w;
    uint8_t *b = (uint8_t *)p;
    w.tile_sums = (Sum2 *)b;
    b += n_tiles_of(n_rec) * sizeof(Sum2);
    w.state = (unsigned long long *)b;
    b += kStateWords * 8;
    w.item_off = (uint64_t *)b;
    b += (n_rec + 1) * 8;
    w.info = (Info *)b;
    b += n_rec * sizeof(Info);
    w.item_rec = (uint32_t *)b;
    w.item_cap = item_bound(n_rec, bytes);
    return w;
}

// the most bytes the records of n_text bytes of text can take.  Per record, with T its text length, H >= name >= 1 and L its bases:
//   FASTA  T = H + L + 3, BAM = 37 + name + ceil(L/2) + L:  BAM - T = 34 + name - H + ceil(L/2) <= 34 + ceil(L/2), and L <= T - 4
//          gives ceil(L/2) <= (T - 3) / 2 <= T / 2;
//   FASTQ  T = H + 2L + 6:  BAM - T = 31 + name - H + ceil(L/2) - L <= 31 (L = 0 and L = 1 reach it with H == name).
// So BAM <= T + T / 2 + 34 for either kind, and the sum over the records is at most n_text + n_text / 2 + 34 n_records (the sum of
// the floors is at most the floor of the sum).  A FASTA record of L = 0 with a 1-byte name has T = 4 and BAM = 38 <= 4 + 2 + 34.
uint64_t enc_bound(uint64_t n_text, uint64_t n_records) { return n_text + n_text / 2 + 34 * n_records; }

}  // namespace

size_t flx_bam_encode_work_bytes(uint64_t n_rec, uint64_t bytes) {
    return (size_t)(n_tiles_of(n_rec) * sizeof(Sum2) + kStateWords * 8 + (n_rec + 1) * 8 + n_rec * sizeof(Info) + item_bound(n_rec, bytes) * 4 + 64);
}

unsigned flx_bam_encode_blocks(const flx_ctx *ctx) {
    return (unsigned)(ctx->prop.multiProcessorCount > 0 ? ctx->prop.multiProcessorCount : 256) * kEmitBlocksPerCU;
}

// The launches of one call on `st` (n_rec >= 1; `work` has flx_bam_encode_work_bytes(n_rec, n) bytes or more, carved for exactly
// (n_rec, n)): h_state (pinned, or read after a synchronisation) gets [0] the BAM bytes and [3] n_rec - the lowest bad record.
hipError_t flx_bam_encode_launch(hipStream_t st, unsigned emit_blocks, const void *d_text, uint64_t n, const uint64_t *d_off, uint64_t n_rec,
                                 void *work, uint64_t *d_out_off, void *d_out, uint64_t out_cap, uint64_t *h_state) {
    const EncWork w = carve(work, n_rec, n);
    hipError_t e = hipMemsetAsync(w.state, 0, kStateWords * 8, st);
    if (e != hipSuccess) return e;
    const uint64_t tiles = n_tiles_of(n_rec);
    const uint8_t *text = (const uint8_t *)d_text;
    hipLaunchKernelGGL(k_bamenc_sizes, dim3((unsigned)tiles), dim3(ENC_NT), 0, st, text, n, d_off, n_rec, w.info, w.tile_sums, w.state);
    hipLaunchKernelGGL(k_bamenc_scan_tiles, dim3(1), dim3(ENC_NT), 0, st, w.tile_sums, tiles, w.state);
    hipLaunchKernelGGL(k_bamenc_offsets, dim3((unsigned)tiles), dim3(ENC_NT), 0, st, text, d_off, n_rec, w.info, w.tile_sums, w.state, d_out_off,
                       w.item_off, w.item_rec, w.item_cap);
    const uint64_t blocks = w.item_cap < emit_blocks ? w.item_cap : emit_blocks;
    hipLaunchKernelGGL(k_bamenc_emit, dim3((unsigned)(blocks ? blocks : 1)), dim3(ENC_NT), 0, st, text, d_off, n_rec, w.info, d_out_off, w.item_off,
                       w.item_rec, w.item_cap, w.state, (uint8_t *)d_out, out_cap);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    return hipMemcpyAsync(h_state, w.state, kStateWords * 8, hipMemcpyDeviceToHost, st);
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
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return flx_fail(ctx, FLX_ERR_HIP, "flx_bam_from_fastq_dev: %s", hipGetErrorString(e));
    *first_bad = n_records - (st[3] <= n_records ? st[3] : n_records);
    *out_len = st[0];
    if (st[0] > out_cap)
        return flx_fail(ctx, FLX_ERR_CAPACITY, "flx_bam_from_fastq_dev: %llu bytes needed, capacity %llu", (unsigned long long)st[0],
                        (unsigned long long)out_cap);
    return FLX_OK;
}
