// bgzf.hip — BGZF compression on the GPU: gzip members of at most 65280 input bytes, each with the BC extra field
// (SAM/BAM specification §4.1), optionally followed by the 28-byte end-of-file block.
//
// k_bgzf_members   one workgroup per member (the phases of bgzf_member.h): the compressed member in a 65664-byte slot;
// k_bgzf_scan      exclusive scan of the members' sizes of one batch onto the running total (and the capacity check);
// k_bgzf_gather    one workgroup per member: its bytes into the contiguous output;
// k_bgzf_eof       the end-of-file block.
// A call runs the members in batches of at most kBatch (the match table of a batch lives in device scratch); everything stays
// in stream order, the host reads back 16 bytes at the end.  The output is a pure function of (bytes, flags).
#include <condition_variable>
#include <mutex>

#include "flx_internal.h"
#include "bgzf_member.h"
#include "host_pieces.h"

using namespace bgzf;

namespace {

constexpr uint32_t kBatch = 1024;   // members per launch (k_bgzf_scan scans one batch with one workgroup)
constexpr int kScanThreads = 1024;

const uint8_t kEof[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};

struct Work {  // device scratch of one call
    uint64_t *state;  // [0] bytes so far (needed size), [1] capacity exceeded
    uint32_t *sizes;  // [kBatch]
    uint64_t *offs;   // [kBatch]
    uint8_t *slots;   // [batch * BG_SLOT]
    uint32_t *mt;     // [batch * BG_MEMBER]
};

size_t work_bytes(uint64_t n) {
    const uint64_t members = (n + BG_MEMBER - 1) / BG_MEMBER;
    const uint64_t b = members < kBatch ? members : kBatch;
    return 256 + 4 * kBatch + 8 * kBatch + b * BG_SLOT + b * BG_MEMBER * 4;
}

Work carve(void *p, uint64_t n) {
    const uint64_t members = (n + BG_MEMBER - 1) / BG_MEMBER;
    const uint64_t b = members < kBatch ? members : kBatch;
    uint8_t *c = (uint8_t *)p;
    Work w;
    w.state = (uint64_t *)c;
    w.sizes = (uint32_t *)(c + 256);
    w.offs = (uint64_t *)(c + 256 + 4 * kBatch);
    w.slots = c + 256 + 12 * kBatch;
    w.mt = (uint32_t *)(w.slots + b * BG_SLOT);
    return w;
}

__global__ void __launch_bounds__(BG_NT) k_bgzf_members(const uint8_t *in, uint64_t n_total, uint64_t first_member,
                                                        uint32_t *mt, uint8_t *slots, uint32_t *sizes) {
    __shared__ Shared S;
    const int t = threadIdx.x;
    const uint64_t off = (first_member + blockIdx.x) * (uint64_t)BG_MEMBER;
    const uint32_t n = n_total - off < BG_MEMBER ? (uint32_t)(n_total - off) : BG_MEMBER;
    const uint8_t *src = in + off;
    uint32_t *m = mt + (size_t)blockIdx.x * BG_MEMBER;
    uint8_t *slot = slots + (size_t)blockIdx.x * BG_SLOT;

    ph_load(t, S, src, n, ((uintptr_t)src & 15) == 0);
    __syncthreads();
    ph_crc(t, S, n);
    __syncthreads();
    ph_crc_final(t, S, n);
    for (uint32_t base = 0; base < n; base += BG_NT) {
        ph_lookup(t, S, n, base, m);
        __syncthreads();
        ph_insert(t, S, n, base);
        __syncthreads();
    }
    ph_hist(t, S, n, m);
    __syncthreads();
    ph_rank(t, S);
    __syncthreads();
    ph_codes(t, S);
    __syncthreads();
    ph_header(t, S, n);
    __syncthreads();
    ph_count(t, S, n, m);
    __syncthreads();
    ph_scan(t, S);
    __syncthreads();
    ph_zero(t, S, slot);
    __syncthreads();
    ph_pack(t, S, n, m, slot);
    __syncthreads();
    ph_frame(t, S, n, slot, sizes + blockIdx.x);
}

// offs[k] = running total + sizes of the members before k; the running total moves on; past `cap` the flag is set for good
__global__ void __launch_bounds__(kScanThreads) k_bgzf_scan(const uint32_t *sizes, uint32_t m, uint64_t *offs, uint64_t *state,
                                                            uint64_t cap) {
    __shared__ uint32_t s[kScanThreads];
    __shared__ uint64_t base;
    const int t = threadIdx.x;
    const uint32_t v = (uint32_t)t < m ? sizes[t] : 0;
    s[t] = v;
    if (t == 0) base = state[0];
    __syncthreads();
    for (int d = 1; d < kScanThreads; d <<= 1) {
        const uint32_t a = t >= d ? s[t - d] : 0;
        __syncthreads();
        s[t] += a;
        __syncthreads();
    }
    if ((uint32_t)t < m) offs[t] = base + s[t] - v;
    if (t == 0) {
        const uint64_t total = base + s[kScanThreads - 1];
        if (total > cap) state[1] = 1;
        state[0] = total;
    }
}

__global__ void __launch_bounds__(256) k_bgzf_gather(const uint8_t *slots, const uint32_t *sizes, const uint64_t *offs,
                                                     const uint64_t *state, uint8_t *out) {
    if (state[1]) return;  // capacity exceeded: nothing is written
    const uint8_t *slot = slots + (size_t)blockIdx.x * BG_SLOT;
    const uint32_t sz = sizes[blockIdx.x];
    uint8_t *dst = out + offs[blockIdx.x];
    for (uint32_t j = threadIdx.x; j < sz; j += 256) dst[j] = j < 18 ? slot[j] : slot[BG_DEFL_OFF + j - 18];
}

struct EofBlock {
    uint8_t b[28];
};

__global__ void k_bgzf_eof(uint64_t *state, uint8_t *out, uint64_t cap, EofBlock e) {
    const uint64_t at = state[0];
    if (threadIdx.x == 0) {
        if (at + 28 > cap) state[1] = 1;
        if (!state[1])
            for (int k = 0; k < 28; ++k) out[at + k] = e.b[k];
        state[0] = at + 28;
    }
}

// every launch of one call, on `st`; *h_state (host) gets the needed size and the capacity flag
hipError_t bgzf_run(hipStream_t st, const uint8_t *d_in, uint64_t n, int flags, uint8_t *d_out, uint64_t cap, void *work,
                    uint64_t *h_state) {
    Work w = carve(work, n);
    hipError_t e = hipMemsetAsync(w.state, 0, 16, st);
    if (e != hipSuccess) return e;
    const uint64_t members = (n + BG_MEMBER - 1) / BG_MEMBER;
    for (uint64_t first = 0; first < members; first += kBatch) {
        const uint32_t b = (uint32_t)(members - first < kBatch ? members - first : kBatch);
        hipLaunchKernelGGL(k_bgzf_members, dim3(b), dim3(BG_NT), 0, st, d_in, n, first, w.mt, w.slots, w.sizes);
        hipLaunchKernelGGL(k_bgzf_scan, dim3(1), dim3(kScanThreads), 0, st, w.sizes, b, w.offs, w.state, cap);
        hipLaunchKernelGGL(k_bgzf_gather, dim3(b), dim3(256), 0, st, w.slots, w.sizes, w.offs, w.state, d_out);
    }
    if (flags & FLX_BGZF_EOF) {
        EofBlock eb;
        memcpy(eb.b, kEof, 28);
        hipLaunchKernelGGL(k_bgzf_eof, dim3(1), dim3(64), 0, st, w.state, d_out, cap, eb);
    }
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = hipMemcpyAsync(h_state, w.state, 16, hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
    return hipStreamSynchronize(st);
}

uint64_t bound_of(uint64_t n, int flags) {
    return n + 31 * ((n + BG_MEMBER - 1) / BG_MEMBER) + ((flags & FLX_BGZF_EOF) ? 28 : 0);
}

}  // namespace

extern "C" int flx_bgzf_bound(uint64_t n, int flags, uint64_t *bound) {
    if (!bound || (flags & ~FLX_BGZF_EOF)) return FLX_ERR_INVALID;
    *bound = bound_of(n, flags);
    return FLX_OK;
}

extern "C" int flx_bgzf_compress_dev(flx_ctx *ctx, const void *d_in, uint64_t n, int flags, void *d_out, uint64_t out_cap,
                                     uint64_t *out_len) {
    if (!ctx) return FLX_ERR_INVALID;
    if ((!d_in && n) || !out_len || (flags & ~FLX_BGZF_EOF) || (!d_out && out_cap))
        return flx_fail(ctx, FLX_ERR_INVALID, "flx_bgzf_compress_dev: bad argument");
    *out_len = 0;
    void *work = nullptr;
    FLX_CHECK(flx_scratch(ctx, work_bytes(n), &work));
    uint64_t st[2] = {0, 0};
    flx_time_scope ts(ctx, "flx_bgzf");
    hipError_t e = bgzf_run(ctx->stream, (const uint8_t *)d_in, n, flags, (uint8_t *)d_out, out_cap, work, st);
    ts.end();
    if (e != hipSuccess) return flx_fail(ctx, FLX_ERR_HIP, "flx_bgzf_compress_dev: %s", hipGetErrorString(e));
    if (st[1]) return flx_fail(ctx, FLX_ERR_CAPACITY, "flx_bgzf_compress_dev: %llu bytes needed, capacity %llu",
                               (unsigned long long)st[0], (unsigned long long)out_cap);
    *out_len = st[0];
    return FLX_OK;
}

// ---- host-to-host compressor with its own streams and pinned slots ---------------------------------------------------
struct flx_bgzf_slot {
    hipStream_t stream = nullptr;
    flx_dev_buf d_in, d_out, work;
    flx_pinned_buf h_in, h_out, h_state;
    flx_dev_buf d_tab;  // d_tab / h_tab: inflate's piece offsets, its first bad member, its status words
    flx_pinned_buf h_tab;
    // text -> BAM (flx_bgzf_bam_from_fastq): allocated by the first such call on the slot, each grown alone.  The text of a piece
    // goes through h_in / d_in like the compressor's input; e_h_text / e_d_text exist only behind a record larger than the slot.
    flx_pinned_buf e_h_text, e_h_off, e_h_state;
    flx_dev_buf e_d_text, e_d_bam, e_d_off, e_d_out_off, e_work;
    bool busy = false;
};

// inflate runs a call in pieces of at most kInflatePiece members whose compressed bytes fit d_in and whose bytes fit d_out: both
// are kSlotSlack larger than compression needs, so that a single member of 64 KiB (either way) always fits
constexpr uint64_t kInflatePiece = 4096;
constexpr uint64_t kSlotSlack = 256;
constexpr size_t kTabBytes = (2 * (kInflatePiece + 1) + 1) * 8 + kInflatePiece * 4;

struct flx_bgzf {
    flx_ctx *ctx = nullptr;
    int device = 0;
    uint64_t slot_bytes = 0;  // a multiple of 65280: chunks of one call keep the member grid of the whole input
    std::vector<flx_bgzf_slot> slots;
    std::mutex mu;
    std::condition_variable cv;
};

// (every stream is waited for and destroyed before the slots, and with them their buffers, go)
extern "C" void flx_bgzf_destroy(flx_bgzf *z) {
    if (!z) return;
    (void)hipSetDevice(z->device);
    for (auto &s : z->slots)
        if (s.stream) {
            (void)hipStreamSynchronize(s.stream);
            (void)hipStreamDestroy(s.stream);
        }
    delete z;
}

extern "C" int flx_bgzf_create(flx_ctx *ctx, uint64_t slot_bytes, unsigned slots, flx_bgzf **out) {
    if (!ctx) return FLX_ERR_INVALID;
    if (!out || slots == 0 || slots > 256) return flx_fail(ctx, FLX_ERR_INVALID, "flx_bgzf_create: bad argument");
    *out = nullptr;
    uint64_t sb = slot_bytes / BG_MEMBER * BG_MEMBER;
    if (sb == 0) sb = BG_MEMBER;
    flx_bgzf *z = new flx_bgzf();
    z->ctx = ctx;
    z->device = ctx->device;
    z->slot_bytes = sb;
    z->slots.resize(slots);
    FLX_HIP(ctx, hipSetDevice(ctx->device));
    const uint64_t ob = bound_of(sb, FLX_BGZF_EOF);
    for (auto &s : z->slots) {
        hipError_t e = hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking);
        if (e == hipSuccess)
            e = flx_reserve_all(s.d_in, sb + kSlotSlack, s.d_out, ob + kSlotSlack, s.work, work_bytes(sb), s.h_in, sb + kSlotSlack, s.h_out,
                                ob + kSlotSlack, s.h_state, 16, s.d_tab, kTabBytes, s.h_tab, kTabBytes);
        if (e != hipSuccess) {
            flx_bgzf_destroy(z);
            return flx_fail(ctx, FLX_ERR_NOMEM, "flx_bgzf_create: %s", hipGetErrorString(e));
        }
    }
    *out = z;
    return FLX_OK;
}

static flx_bgzf_slot *take_slot(flx_bgzf *z) {
    flx_bgzf_slot *s = nullptr;
    std::unique_lock<std::mutex> lk(z->mu);
    for (;;) {
        for (auto &c : z->slots)
            if (!c.busy) { s = &c; break; }
        if (s) break;
        z->cv.wait(lk);
    }
    s->busy = true;
    return s;
}
static void give_slot(flx_bgzf *z, flx_bgzf_slot *s) {
    {
        std::lock_guard<std::mutex> lk(z->mu);
        s->busy = false;
    }
    z->cv.notify_one();
}

// Thread-safe like flx_bgzf_compress.  Members [k, k + c) of a piece: compressed bytes in, offsets in, bytes and the first bad
// member out; the call stops behind the first piece that holds a bad member.
extern "C" int flx_bgzf_inflate(flx_bgzf *z, const void *in, const uint64_t *in_off, const uint64_t *out_off, uint64_t n_members,
                                void *out, uint64_t *first_bad) {
    if (!z || !first_bad) return FLX_ERR_INVALID;
    *first_bad = n_members;
    if (n_members == 0) return FLX_OK;
    if (!in || !in_off || !out_off || (!out && out_off[n_members] > out_off[0])) return FLX_ERR_INVALID;
    for (uint64_t k = 0; k < n_members; ++k)
        if (in_off[k + 1] < in_off[k] || out_off[k + 1] < out_off[k]) return FLX_ERR_INVALID;
    const uint64_t in_cap = z->slot_bytes + kSlotSlack, out_cap = bound_of(z->slot_bytes, FLX_BGZF_EOF) + kSlotSlack;
    flx_bgzf_slot *s = take_slot(z);
    hipError_t e = hipSetDevice(z->device);
    uint64_t k = 0, bad = n_members;
    while (e == hipSuccess && k < n_members) {
        uint64_t c = 0;
        while (k + c < n_members && c < kInflatePiece && in_off[k + c + 1] - in_off[k] <= in_cap &&
               out_off[k + c + 1] - out_off[k] <= out_cap)
            ++c;
        if (c == 0) {  // a member beyond 64 KiB is no BGZF member
            bad = k;
            break;
        }
        const uint64_t nin = in_off[k + c] - in_off[k], nout = out_off[k + c] - out_off[k];
        uint64_t *h_in_off = s->h_tab.as<uint64_t>(), *h_out_off = h_in_off + c + 1;
        for (uint64_t j = 0; j <= c; ++j) {
            h_in_off[j] = in_off[k + j] - in_off[k];
            h_out_off[j] = out_off[k + j] - out_off[k];
        }
        uint64_t *d_tab = s->d_tab.as<uint64_t>(), *d_first = d_tab + 2 * (kInflatePiece + 1);
        uint32_t *d_status = (uint32_t *)(d_first + 1);
        memcpy(s->h_in.p, (const uint8_t *)in + in_off[k], nin);
        e = hipMemcpyAsync(s->d_in.p, s->h_in.p, nin, hipMemcpyHostToDevice, s->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(d_tab, h_in_off, (2 * c + 2) * 8, hipMemcpyHostToDevice, s->stream);
        if (e == hipSuccess)
            e = flx_bgzf_inflate_launch(s->stream, s->d_in.p, d_tab, d_tab + c + 1, c, s->d_out.p, d_status, d_first);
        if (e == hipSuccess && nout) e = hipMemcpyAsync(s->h_out.p, s->d_out.p, nout, hipMemcpyDeviceToHost, s->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(s->h_state.p, d_first, 8, hipMemcpyDeviceToHost, s->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
        if (e != hipSuccess) {  // what was enqueued in front of the failure may still read or write the slot's buffers
            (void)hipStreamSynchronize(s->stream);
            break;
        }
        const uint64_t fb = *s->h_state.as<uint64_t>() < c ? *s->h_state.as<uint64_t>() : c;
        memcpy((uint8_t *)out + out_off[k], s->h_out.p, (size_t)(h_out_off[fb]));
        if (fb < c) {
            bad = k + fb;
            break;
        }
        k += c;
    }
    give_slot(z, s);
    if (e != hipSuccess) return FLX_ERR_HIP;
    *first_bad = bad;
    return FLX_OK;
}

// Thread-safe: a call takes a free slot (or waits for one) and runs its chunks on that slot's stream.
extern "C" int flx_bgzf_compress(flx_bgzf *z, const void *in, uint64_t n, int flags, void *out, uint64_t out_cap,
                                 uint64_t *out_len) {
    if (!z || (!in && n) || !out_len || (flags & ~FLX_BGZF_EOF) || (!out && out_cap)) return FLX_ERR_INVALID;
    *out_len = 0;
    flx_bgzf_slot *s = take_slot(z);
    int rc = FLX_OK;
    hipError_t e = hipSetDevice(z->device);
    uint64_t done = 0, len = 0;
    do {
        const uint64_t c = n - done < z->slot_bytes ? n - done : z->slot_bytes;
        const int f = (done + c == n) ? flags : 0;
        if (e == hipSuccess && c) {
            memcpy(s->h_in.p, (const uint8_t *)in + done, c);
            e = hipMemcpyAsync(s->d_in.p, s->h_in.p, c, hipMemcpyHostToDevice, s->stream);
        }
        const uint64_t cap = bound_of(c, f);
        if (e == hipSuccess) e = bgzf_run(s->stream, s->d_in.as(), c, f, s->d_out.as(), cap, s->work.p, s->h_state.as<uint64_t>());
        if (e != hipSuccess) break;
        const uint64_t got = *s->h_state.as<uint64_t>();
        if (got > out_cap - len) {
            rc = FLX_ERR_CAPACITY;
            break;
        }
        if ((e = hipMemcpyAsync(s->h_out.p, s->d_out.p, got, hipMemcpyDeviceToHost, s->stream)) == hipSuccess)
            e = hipStreamSynchronize(s->stream);
        if (e != hipSuccess) break;
        memcpy((uint8_t *)out + len, s->h_out.p, got);
        len += got;
        done += c;
    } while (done < n);
    if (e != hipSuccess) rc = FLX_ERR_HIP;
    give_slot(z, s);
    if (rc == FLX_OK) *out_len = len;
    return rc;
}

// ---- text -> BAM -> BGZF through one slot ---------------------------------------------------------------------------------
// Room on the (idle) slot for a piece of text_bytes of text in n_rec records.  Every buffer grows alone, and only when it is too
// small: a free synchronises the device under the other workers' streams.  Text of at most slot_bytes needs no buffer of its own.
static hipError_t reserve_encoder(flx_bgzf_slot &s, uint64_t slot_bytes, uint64_t text_bytes, uint64_t n_rec) {
    uint64_t bb = 0;
    (void)flx_bam_from_fastq_bound(text_bytes, n_rec, &bb);
    const uint64_t own_text = text_bytes > slot_bytes ? text_bytes + 16 : 0;
    return flx_reserve_all(s.e_h_state, 32, s.e_h_text, own_text, s.e_d_text, own_text, s.e_h_off, (n_rec + 1) * 8, s.e_d_off, (n_rec + 1) * 8,
                           s.e_d_out_off, (n_rec + 1) * 8, s.e_d_bam, bb + kSlotSlack, s.e_work, flx_bam_encode_work_bytes(n_rec, text_bytes));
}

// Thread-safe like flx_bgzf_compress.  A piece is whole records of at most slot_bytes of text (one record when that record is
// larger): its text goes up, the encode kernels write the BAM bytes into the slot's own buffer, and the compressor's kernels run
// over those bytes in slot-sized chunks exactly as flx_bgzf_compress runs them over an uploaded chunk; only compressed bytes come
// back.  The piece's first bad record is known before anything of the piece is compressed.
extern "C" int flx_bgzf_bam_from_fastq(flx_bgzf *z, const void *text, uint64_t n, const uint64_t *rec_off, uint64_t n_records, int flags,
                                       void *out, uint64_t out_cap, uint64_t *out_len, uint64_t *first_bad) {
    if (!z || !out_len || !first_bad || (flags & ~FLX_BGZF_EOF) || (!out && out_cap)) return FLX_ERR_INVALID;
    *out_len = 0;
    *first_bad = n_records;
    if (n_records && (!text || !rec_off || n_records > 0xffffffffull)) return FLX_ERR_INVALID;
    // offsets that leave the text or run backwards: the lowest such record is bad, nothing is uploaded
    for (uint64_t k = 0; k < n_records; ++k)
        if (!(rec_off[k] <= rec_off[k + 1] && rec_off[k + 1] <= n)) {
            *first_bad = k;
            return FLX_OK;
        }
    flx_bgzf_slot *s = take_slot(z);
    int rc = FLX_OK;
    hipError_t e = hipSetDevice(z->device);
    const unsigned emit_blocks = flx_bam_encode_blocks(z->ctx);
    uint64_t k = 0, len = 0, bad = n_records;
    while (e == hipSuccess && rc == FLX_OK && k < n_records) {
        const uint64_t c = flx_piece_records(rec_off, k, n_records, z->slot_bytes), nin = rec_off[k + c] - rec_off[k];
        // (sized for whole slots, so that the pieces of a run find room the first piece made)
        if ((e = reserve_encoder(*s, z->slot_bytes, nin > z->slot_bytes ? nin : z->slot_bytes, c > kPieceMinTable ? c : kPieceMinTable)) != hipSuccess) {
            rc = FLX_ERR_NOMEM;
            break;
        }
        uint8_t *h_text = (nin <= z->slot_bytes ? s->h_in : s->e_h_text).as(), *d_text = (nin <= z->slot_bytes ? s->d_in : s->e_d_text).as();
        const uint64_t bam_cap = s->e_d_bam.cap - kSlotSlack, *e_state = s->e_h_state.as<uint64_t>();
        flx_piece_table(rec_off, k, c, s->e_h_off.as<uint64_t>());
        memcpy(h_text, (const uint8_t *)text + rec_off[k], (size_t)nin);
        if (nin) e = hipMemcpyAsync(d_text, h_text, nin, hipMemcpyHostToDevice, s->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(s->e_d_off.p, s->e_h_off.p, (c + 1) * 8, hipMemcpyHostToDevice, s->stream);
        if (e == hipSuccess)
            e = flx_bam_encode_launch(s->stream, emit_blocks, d_text, nin, s->e_d_off.as<uint64_t>(), c, s->e_work.p, s->e_d_out_off.as<uint64_t>(),
                                      s->e_d_bam.p, bam_cap, s->e_h_state.as<uint64_t>());
        if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
        if (e != hipSuccess) {
            (void)hipStreamSynchronize(s->stream);
            break;
        }
        const uint64_t enc = e_state[0], nbad = e_state[3];
        if (nbad) {
            bad = k + (c - (nbad <= c ? nbad : c));
            break;
        }
        if (enc > bam_cap) {  // (cannot happen: the buffer has the bound of the piece)
            rc = FLX_ERR_STATE;
            break;
        }
        const bool last_piece = k + c == n_records;
        for (uint64_t done = 0; done < enc && rc == FLX_OK;) {
            const uint64_t cb = enc - done < z->slot_bytes ? enc - done : z->slot_bytes;
            const int f = (last_piece && done + cb == enc) ? flags : 0;
            if ((e = bgzf_run(s->stream, s->e_d_bam.as() + done, cb, f, s->d_out.as(), bound_of(cb, f), s->work.p, s->h_state.as<uint64_t>())) != hipSuccess) break;
            const uint64_t got = *s->h_state.as<uint64_t>();
            if (got > out_cap - len) {
                rc = FLX_ERR_CAPACITY;
                break;
            }
            if ((e = hipMemcpyAsync(s->h_out.p, s->d_out.p, got, hipMemcpyDeviceToHost, s->stream)) == hipSuccess) e = hipStreamSynchronize(s->stream);
            if (e != hipSuccess) break;
            memcpy((uint8_t *)out + len, s->h_out.p, (size_t)got);
            len += got;
            done += cb;
        }
        k += c;
    }
    // (the end-of-file block of a call whose last piece held no byte to carry it: no records at all)
    if (e == hipSuccess && rc == FLX_OK && bad == n_records && n_records == 0 && (flags & FLX_BGZF_EOF)) {
        if (out_cap < 28) rc = FLX_ERR_CAPACITY;
        else {
            memcpy(out, kEof, 28);
            len = 28;
        }
    }
    give_slot(z, s);
    if (e != hipSuccess && rc == FLX_OK) rc = FLX_ERR_HIP;
    if (rc != FLX_OK) return rc;
    *first_bad = bad;
    if (bad == n_records) *out_len = len;
    return FLX_OK;
}