// bam.hip — unaligned BAM records turned into FASTQ text on the GPU: the layer inside the BGZF container of bgzf_inflate.hip.
//
// flx_bam_index         (host) the header and the chain of block_size fields: one load per record, serial, so it stays on the host;
// the layout pass       (record_pipeline.h) with the Decode codec below: a record is validated (bam_record.h: read_record) and
//                       gives its text size, its number of emit items and whether it is skipped;
// k_bam_emit            one workgroup per (record, chunk of BAM_CHUNK bases), grid-stride over the items: a 4 Mbp record is a
//                       thousand items spread over the chip, a 200-base record is one.
// The emit kernel moves ~1.5 bytes in and 2 bytes out per base.  Output positions fall on every alignment, so each of the two
// lines of a chunk is written as head bytes up to the next 16-byte boundary of the OUTPUT address, whole aligned 16-byte stores
// (one lane each: 16 bases from 8 or 9 packed bytes through a 256-entry table of character pairs in LDS, 16 qualities clamped four
// to a word), and tail bytes.  Loads take exactly the bytes they need at whatever address they lie (the hardware's unaligned
// global loads): nothing outside a record is read, and a record was validated against its own range by the layout pass.
#include "flx_internal.h"
#include "bam_record.h"
#include "host_pieces.h"
#include "record_pipeline.h"

using namespace bam;
using recpipe::kStateWords;

namespace {

constexpr int BAM_NT = recpipe::NT;             // threads per workgroup
constexpr uint32_t BAM_CHUNK = recpipe::CHUNK;  // bases per emit item: one 16-byte store per lane and line

// what record k of the index gives: zero sums and bad for a record that is not valid inside [off[k], off[k+1]) of in[0, n)
struct Decode {
    using Sums = recpipe::Sum3;
    static size_t extra_bytes(uint64_t n_rec) { return (n_rec + 1) * 8; }  // text offsets of a call that has no array for them
    const uint8_t *in;
    uint64_t n;
    const uint64_t *off;
    __device__ __forceinline__ Sums measure(uint64_t k, bool *bad) const {
        const uint64_t at = off[k], end = off[k + 1];
        Rec r;
        *bad = !(at <= end && end <= n) || read_record(in, end, at, r) != REC_OK || r.end != end;
        if (*bad) return {0, 0, 0};
        const uint64_t bytes = text_size(r);
        return {bytes, bytes ? ((uint64_t)r.l_seq + BAM_CHUNK - 1) / BAM_CHUNK : 0, bytes ? 0ull : 1ull};
    }
    __device__ __forceinline__ Sums recall(uint64_t k) const {
        bool bad;
        return measure(k, &bad);
    }
};

// 16 bases whose first is base i of the record, as the 8 packed bytes that hold them in order (byte m: bases i + 2m, i + 2m + 1)
__device__ __forceinline__ uint64_t load_bases16(const uint8_t *seq, uint64_t i) {
    const uint8_t *p = seq + (i >> 1);
    uint64_t w;
    __builtin_memcpy(&w, p, 8);
    if (i & 1) {  // shifted by a nibble: byte m = low nibble of p[m], high nibble of p[m + 1]
        const uint64_t next = (w >> 8) | (uint64_t)p[8] << 56;
        w = ((w << 4) & 0xf0f0f0f0f0f0f0f0ull) | ((next >> 4) & 0x0f0f0f0f0f0f0f0full);
    }
    return w;
}

__device__ __forceinline__ uint32_t bswap32(uint32_t x) { return __builtin_bswap32(x); }

// min(q, 93) + 33 on the four bytes of a word
__device__ __forceinline__ uint32_t qual_chars4(uint32_t x) {
    const uint32_t over = (((x & 0x7f7f7f7fu) + 0x22222222u) | x) & 0x80808080u;  // bit 7 of every byte >= 94
    const uint32_t m = (over >> 7) * 0xffu;
    return ((x & ~m) | (0x5d5d5d5du & m)) + 0x21212121u;
}

// One line (SEQ or QUAL) of a chunk: characters [b0, b0 + len) of the line go to dst[0, len).
template <bool QUAL>
__device__ __forceinline__ void emit_line(const uint8_t *in, const Rec &r, uint64_t b0, uint32_t len, uint8_t *dst, const uint16_t (*lut)[256]) {
    const uint32_t t = threadIdx.x;
    const bool rev = r.flag & FLAG_REVERSE;
    const uint64_t l = (uint64_t)r.l_seq;
    const auto [head, groups, tail] = recpipe::split16(dst, len);
    if (t < head) dst[t] = QUAL ? qual_char_at(in, r, b0 + t) : seq_char_at(in, r, b0 + t);
    if (t < tail) {
        const uint32_t j = head + 16 * groups + t;
        dst[j] = QUAL ? qual_char_at(in, r, b0 + j) : seq_char_at(in, r, b0 + j);
    }
    if (t >= groups) return;  // (groups <= BAM_CHUNK / 16 = BAM_NT: one per lane)
    const uint64_t j = b0 + head + 16 * (uint64_t)t;  // the group's first character; j + 16 <= l
    const uint64_t i = rev ? l - 16 - j : j;          // ... is made of bases / qualities [i, i + 16)
    uint4 o;
    if (QUAL) {
        if (in[r.qual] == 0xff) {
            o.x = o.y = o.z = o.w = 0x01010101u * kMissingQual;
        } else {
            uint32_t w[4];
            __builtin_memcpy(w, in + r.qual + i, 16);
            if (rev) {
                const uint32_t a = bswap32(w[3]), b = bswap32(w[2]), c = bswap32(w[1]), d = bswap32(w[0]);
                w[0] = a; w[1] = b; w[2] = c; w[3] = d;
            }
            o.x = qual_chars4(w[0]); o.y = qual_chars4(w[1]); o.z = qual_chars4(w[2]); o.w = qual_chars4(w[3]);
        }
    } else {
        uint64_t w = load_bases16(in + r.seq, i);
        if (rev) w = __builtin_bswap64(w);
        const uint16_t *tab = lut[rev ? 1 : 0];
        o.x = (uint32_t)tab[w & 255] | (uint32_t)tab[(w >> 8) & 255] << 16;
        o.y = (uint32_t)tab[(w >> 16) & 255] | (uint32_t)tab[(w >> 24) & 255] << 16;
        o.z = (uint32_t)tab[(w >> 32) & 255] | (uint32_t)tab[(w >> 40) & 255] << 16;
        o.w = (uint32_t)tab[(w >> 48) & 255] | (uint32_t)tab[(w >> 56) & 255] << 16;
    }
    *(uint4 *)(dst + head + 16 * (uint64_t)t) = o;
}

__global__ void __launch_bounds__(BAM_NT) k_bam_emit(Decode codec, uint64_t n_rec, const uint64_t *out_off, const uint64_t *item_off,
                                                     const uint32_t *item_rec, uint64_t item_cap, unsigned long long *state, uint8_t *out,
                                                     uint64_t out_cap) {
    const uint8_t *in = codec.in;
    const uint64_t *off = codec.off;
    __shared__ uint16_t lut[2][256];
    const uint32_t t = threadIdx.x;
    lut[0][t] = pair_chars(t, false);
    lut[1][t] = pair_chars(t, true);
    __syncthreads();
    const uint64_t n_items = state[1] < item_cap ? state[1] : item_cap;
    if (state[0] > out_cap) return;  // FLX_ERR_CAPACITY: nothing is written
    for (uint64_t w = blockIdx.x; w < n_items; w += gridDim.x) {
        const uint64_t k = item_rec[w];
        if (k >= n_rec || item_off[k] > w) continue;  // (cannot happen: k_offsets wrote the item)
        Rec r;
        if (read_record(in, off[k + 1], off[k], r) != REC_OK || !has_text(r)) continue;  // (cannot happen: the item exists)
        const uint64_t c = w - item_off[k];
        const uint64_t o = out_off[k], l = (uint64_t)r.l_seq;
        if (c * BAM_CHUNK >= l || o + text_size(r) > out_cap) continue;
        uint8_t *seq_line = out + o + r.l_name + 1, *qual_line = seq_line + l + 3;
        if (c == 0) {  // the record's edges
            if (t == 0) {
                out[o] = '@';
                seq_line[-1] = '\n';
                seq_line[l] = '\n';
                seq_line[l + 1] = '+';
                seq_line[l + 2] = '\n';
                qual_line[l] = '\n';
            }
            for (uint32_t i = t; i + 1 < r.l_name; i += BAM_NT) out[o + 1 + i] = in[r.name + i];
        }
        const uint64_t b0 = c * BAM_CHUNK;
        const uint32_t len = (uint32_t)(l - b0 < BAM_CHUNK ? l - b0 : BAM_CHUNK);
        emit_line<false>(in, r, b0, len, seq_line + b0, lut);
        emit_line<true>(in, r, b0, len, qual_line + b0, lut);
    }
}

}  // namespace

extern "C" int flx_bam_index(const void *bam, uint64_t n, uint64_t max_records, uint64_t *rec_off, uint64_t *n_records, int *end_state) {
    if ((!bam && n) || !n_records || !end_state) return FLX_ERR_INVALID;
    *end_state = index_host((const uint8_t *)bam, n, max_records, rec_off, n_records);
    return FLX_OK;
}

extern "C" int flx_bam_to_fastq_dev(flx_ctx *ctx, const void *d_bam, uint64_t n, const uint64_t *d_rec_off, uint64_t n_records, void *d_out,
                                    uint64_t out_cap, uint64_t *d_out_off, uint64_t *out_len, uint64_t *n_skipped, uint64_t *first_bad) {
    if (!ctx) return FLX_ERR_INVALID;
    if (!out_len || !n_skipped || !first_bad) return flx_fail(ctx, FLX_ERR_INVALID, "flx_bam_to_fastq_dev: bad argument");
    *out_len = 0;
    *n_skipped = 0;
    *first_bad = n_records;
    if (n_records == 0) return FLX_OK;
    if (!d_bam || !d_rec_off || !d_out_off || (!d_out && out_cap) || n_records > 0xffffffffull)
        return flx_fail(ctx, FLX_ERR_INVALID, "flx_bam_to_fastq_dev: bad argument");
    void *work = nullptr;
    FLX_CHECK(flx_scratch(ctx, recpipe::work_bytes<Decode>(n_records, n), &work));
    uint64_t st[kStateWords] = {0, 0, 0, 0};
    flx_time_scope ts(ctx, "flx_bam");
    const hipError_t e = recpipe::launch(ctx->stream, recpipe::emit_blocks_of(ctx), Decode{(const uint8_t *)d_bam, n, d_rec_off}, n_records,
                                         recpipe::carve<Decode>(work, n_records, n), d_out_off, k_bam_emit, d_out, out_cap, st);
    ts.end();
    const int rc = recpipe::finish_dev(ctx, "flx_bam_to_fastq_dev", e, st, n_records, out_cap, out_len, first_bad);
    if (rc == FLX_OK || rc == FLX_ERR_CAPACITY) *n_skipped = st[2];
    return rc;
}

// ---- host to host: pieces of whole records through two pinned slots ------------------------------------------------------------
namespace {

struct BamSlot {
    hipStream_t stream = nullptr;
    flx_pinned_buf h_in, h_out, h_tab, h_state;  // h_tab / d_tab: the piece's record offsets (relative to its first byte)
    flx_dev_buf d_in, d_out, d_tab, work;
    uint64_t in_cap = 0, rec_cap = 0;
    // the piece in flight
    bool pending = false;
    uint64_t k0 = 0, k1 = 0, out_at = 0, want = 0, skipped = 0;

    // room for a piece of in_bytes and n_rec records (the slot is idle); the text of a piece is at most twice its bytes
    hipError_t reserve(uint64_t in_bytes, uint64_t n_rec) {
        const uint64_t ib = in_bytes > in_cap ? in_bytes : in_cap, nr = n_rec > rec_cap ? n_rec : rec_cap;
        const hipError_t e = flx_reserve_all(h_in, ib, h_out, 2 * ib, d_in, ib, d_out, 2 * ib, h_tab, (nr + 1) * 8, d_tab, (nr + 1) * 8,
                                             work, recpipe::work_bytes<Decode>(nr, ib));
        if (e == hipSuccess) in_cap = ib, rec_cap = nr;
        return e;
    }
    ~BamSlot() {  // (the buffers are freed behind this: nothing of the stream still uses them)
        if (stream) {
            (void)hipStreamSynchronize(stream);
            (void)hipStreamDestroy(stream);
        }
    }
};

}  // namespace

extern "C" int flx_bam_to_fastq(flx_ctx *ctx, const void *bam, uint64_t n, const uint64_t *rec_off, uint64_t n_records, uint64_t piece_bytes,
                                void *out, uint64_t out_cap, uint64_t *out_off, uint64_t *out_len, uint64_t *n_skipped, uint64_t *first_bad) {
    if (!ctx) return FLX_ERR_INVALID;
    if (!out_len || !n_skipped || !first_bad) return flx_fail(ctx, FLX_ERR_INVALID, "flx_bam_to_fastq: bad argument");
    *out_len = 0;
    *n_skipped = 0;
    *first_bad = n_records;
    if (out_off) out_off[0] = 0;
    if (n_records == 0) return FLX_OK;
    if (!bam || !rec_off || (!out && out_cap) || n_records > 0xffffffffull) return flx_fail(ctx, FLX_ERR_INVALID, "flx_bam_to_fastq: bad argument");
    const uint8_t *src = (const uint8_t *)bam;
    // The host knows what the device will say: it reads every record's fixed fields with the same read_record while it cuts the
    // pieces (one cache line per record), so the copy back of a piece is enqueued with its length and no piece waits for a
    // synchronisation.  What the device finds is compared with it when the piece comes back.
    uint64_t good = 0, need = 0;
    for (; good < n_records; ++good) {
        Rec r;
        const uint64_t at = rec_off[good], end = rec_off[good + 1];
        if (!(at <= end && end <= n) || read_record(src, end, at, r) != REC_OK || r.end != end) break;
        if (out_off) out_off[good + 1] = need + text_size(r);
        need += text_size(r);
        *n_skipped += !has_text(r);
    }
    *first_bad = good;
    if (need > out_cap) {
        *out_len = need;
        return flx_fail(ctx, FLX_ERR_CAPACITY, "flx_bam_to_fastq: %llu bytes needed, capacity %llu", (unsigned long long)need, (unsigned long long)out_cap);
    }
    if (piece_bytes == 0) piece_bytes = 32ull << 20;
    FLX_HIP(ctx, hipSetDevice(ctx->device));
    BamSlot slots[2];
    for (BamSlot &s : slots) {
        FLX_HIP(ctx, hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking));
        FLX_HIP(ctx, s.h_state.reserve(kStateWords * 8));
    }
    const unsigned emit_blocks = recpipe::emit_blocks_of(ctx);
    uint8_t *dst = (uint8_t *)out;
    // the piece of a slot comes back: its text to its place, and the device's word against the host's
    auto finish = [&](BamSlot &s) -> int {
        if (!s.pending) return FLX_OK;
        s.pending = false;
        FLX_HIP(ctx, hipStreamSynchronize(s.stream));
        const uint64_t *st = s.h_state.as<uint64_t>();
        if (st[0] != s.want || st[2] != s.skipped || st[3] != 0)
            return flx_fail(ctx, FLX_ERR_STATE, "flx_bam_to_fastq: the device disagrees with the host about records %llu..%llu",
                            (unsigned long long)s.k0, (unsigned long long)s.k1);
        if (s.want) memcpy(dst + s.out_at, s.h_out.p, (size_t)s.want);
        return FLX_OK;
    };
    uint64_t k = 0, out_at = 0;
    unsigned p = 0;  // pieces alternate between the slots, so the older of two in flight is the one the next piece would take
    for (; k < good; ++p) {
        BamSlot &s = slots[p & 1];
        FLX_CHECK(finish(s));
        const uint64_t c = flx_piece_records(rec_off, k, good, piece_bytes), nin = rec_off[k + c] - rec_off[k];
        hipError_t e = s.reserve(nin > piece_bytes ? nin : piece_bytes, c > kPieceMinTable ? c : kPieceMinTable);
        if (e != hipSuccess) return flx_fail(ctx, FLX_ERR_NOMEM, "flx_bam_to_fastq: %s", hipGetErrorString(e));
        flx_piece_table(rec_off, k, c, s.h_tab.as<uint64_t>());
        memcpy(s.h_in.p, src + rec_off[k], (size_t)nin);
        s.k0 = k;
        s.k1 = k + c;
        s.out_at = out_at;
        s.want = text_bytes_host(src, rec_off, k, k + c, &s.skipped);
        const auto w = recpipe::carve<Decode>(s.work.p, s.rec_cap, s.in_cap);
        e = hipMemcpyAsync(s.d_in.p, s.h_in.p, nin, hipMemcpyHostToDevice, s.stream);
        if (e == hipSuccess) e = hipMemcpyAsync(s.d_tab.p, s.h_tab.p, (c + 1) * 8, hipMemcpyHostToDevice, s.stream);
        if (e == hipSuccess)
            e = recpipe::launch(s.stream, emit_blocks, Decode{s.d_in.as(), nin, s.d_tab.as<uint64_t>()}, c, w, (uint64_t *)w.extra, k_bam_emit,
                                s.d_out.p, 2 * s.in_cap, s.h_state.as<uint64_t>());
        if (e == hipSuccess && s.want) e = hipMemcpyAsync(s.h_out.p, s.d_out.p, s.want, hipMemcpyDeviceToHost, s.stream);
        s.pending = true;  // (whatever was enqueued is waited for: finish, or the slot's destructor)
        if (e != hipSuccess) return flx_fail(ctx, FLX_ERR_HIP, "flx_bam_to_fastq: %s", hipGetErrorString(e));
        out_at += s.want;
        k += c;
    }
    FLX_CHECK(finish(slots[p & 1]));
    FLX_CHECK(finish(slots[(p & 1) ^ 1]));
    *out_len = out_at;
    return FLX_OK;
}