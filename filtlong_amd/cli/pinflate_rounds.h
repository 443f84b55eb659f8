// pinflate_rounds.h — one round of the parallel gzip reader: from a position in the file (Cursor) to what was decoded from there and
// where the next round begins (Result).  A round changes nothing but its Result and the scratch it works in (decoders, buffer pool),
// so a round that cannot finish — an allocation that fails — simply never happened: zlib reads on from the cursor it started at.
//
// BGZF members (SAM specification 4.1) name their own size: a round inflates runs of them side by side, through zlib or through the
// device inflater.  Any other member is one deflate stream, which can only be decoded from a block boundary and with the 32 KiB of
// output in front of it — neither is known in the middle of a file.  The technique is the one published with pugz / rapidgzip:
//   1. the compressed bytes are cut into chunks; each thread SEARCHES its chunk, bit by bit, for the start of a dynamic-Huffman
//      block: a header whose three code sets are complete and not over-subscribed, followed by a block that decodes to text;
//   2. it decodes from there with an UNKNOWN window (deflate_markers.h): a back-reference that reaches in front of the chunk becomes
//      a marker "byte w of the window" and is copied around like a literal;
//   3. a chunk stops at the block boundary where the next chunk's decoding began.  The decoding of chunk i runs through every true
//      block boundary, so a chunk whose start it meets exactly was started at a true boundary and its symbols are the true ones; a
//      start it runs past was a false positive and that chunk's work is dropped;
//   4. along the chain of chunks the windows are resolved one after the other (32 KiB each), then all markers are replaced and the
//      CRC-32 of every chunk computed on all threads; the member's CRC-32 and size are checked against the trailer.
// Every chain boundary is an access point (GzPoint) for the concurrent output pass, exactly as the serial reader leaves them.
// Whatever these decoders cannot do or do not like (a chunk that fails, a stream they find corrupt, a small member) goes to zlib
// from the last boundary: zlib has the last word on every byte that is not plainly decodable.
#pragma once
#include <zlib.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "../../include/filtlong_hip.h"
#include "../csrc/gzip_framing.h"
#include "deflate_markers.h"
#include "inflate_stream.h"
#include "pinflate_queue.h"

namespace pinflate {

inline size_t min_bytes() {  // smaller files (and members behind the first) are not worth the threads
    if (const char *e = getenv("FLX_CLI_PINFLATE_MIN")) return (size_t)atoll(e);
    return (size_t)8 << 20;
}
inline size_t chunk_bytes() {  // compressed bytes per chunk (tests force tiny chunks)
    if (const char *e = getenv("FLX_CLI_PINFLATE_CHUNK")) return std::max<size_t>(64, (size_t)atoll(e));
    return (size_t)2 << 20;
}

// body(0) .. body(n - 1) on up to `threads` threads.  A worker that threw (an allocation that failed) does not end the process:
// the others finish, then std::bad_alloc leaves from here.
template <class F>
static void run_parallel(size_t n, unsigned threads, F &&body) {
    std::atomic<bool> ok{true};
    auto guarded = [&](size_t i) {
        try { body(i); } catch (...) { ok = false; }
    };
    if (n <= 1 || threads <= 1) {
        for (size_t i = 0; i < n; ++i) guarded(i);
    } else {
        std::vector<std::thread> th;
        const unsigned t = (unsigned)std::min<size_t>(threads, n);
        for (unsigned k = 0; k < t; ++k) th.emplace_back([&, k] { for (size_t i = k; i < n; i += t) guarded(i); });
        for (auto &x : th) x.join();
    }
    if (!ok) throw std::bad_alloc();
}

// the producer's position in the file
struct Cursor {
    bool bgzf = false;         // the next round takes BGZF members from bgzf_at; else chunks of one member from chain_bit
    size_t bgzf_at = 0;
    uint64_t stream_out = 0;   // bytes decoded so far
    uint64_t chain_bit = 0;    // a block boundary of the current member, of which ...
    uint64_t member_base = 0;  // ... the first byte is this stream offset,
    uint64_t member_out = 0;   // ... this many bytes are decoded, with this CRC-32,
    uLong crc = 0;
    std::string window;        // ... and these are the last 32 KiB
};

struct Counters {
    uint64_t parallel_bytes = 0, zlib_tail_bytes = 0, device_members = 0, device_handed = 0, device_ns = 0;
    unsigned rounds = 0, dropped_chunks = 0;
};

struct Result {
    enum End { GO_ON, FINISHED, ERROR /* the stream is damaged: `deliverable` */, HAND_OVER /* zlib reads on at `handover` */ };
    End end = GO_ON;
    Batch batch;     // what the round decoded
    Counters add;
    Cursor next;     // (GO_ON) where the next round begins
    uint64_t deliverable = 0;
    GzPoint handover;
    Result() = default;
    explicit Result(const Cursor &from) : next(from) {}
};

// a member starts at byte `in`, stream offset `out`: the point from which zlib (or the output pass) reads header and all
static inline GzPoint member_point(uint64_t in, uint64_t out) {
    GzPoint pt;  // (raw = false)
    pt.in = in;
    pt.out = out;
    return pt;
}
// Inside the member of `c`, at block boundary `bit`, `out` bytes into the member.  check: a hand-over to zlib — c.crc covers the
// member's bytes in front of the point, and whoever inflates on verifies the trailer (an access point of the output pass re-reads
// validated bytes: no check)
static inline GzPoint point_at(const Cursor &c, uint64_t bit, uint64_t out, const std::string &window, bool check = false) {
    GzPoint pt;
    pt.raw = true;
    pt.out = c.member_base + out;
    pt.in = (bit + 7) >> 3;
    pt.bits = (int)((8 - (bit & 7)) & 7);
    pt.window = window;
    pt.check = check;
    pt.member_base = c.member_base;
    pt.crc = c.crc;
    return pt;
}

class Rounds {
public:
    void init(const unsigned char *data, size_t size, unsigned threads, flx_bgzf *device, bool zlib_tails, BufferPool *pool) {
        data_ = data; size_ = size; threads_ = threads; gpu_ = device; zlib_tails_ = zlib_tails; pool_ = pool;
        decoders_.resize(threads);
    }

    // zlib reads on from pt (done by the reading thread once it has taken everything decoded before it)
    void hand_over(Result &r, const GzPoint &pt) const {
        r.end = Result::HAND_OVER;
        r.handover = pt;
        if (gpu_) ++r.add.device_handed;  // (the member at pt.in)
    }
    // where zlib reads on when the round from c could not be made
    GzPoint point_of(const Cursor &c) const {
        return c.bgzf ? member_point(c.bgzf_at, c.stream_out) : point_at(c, c.chain_bit, c.member_out, c.window, true);
    }

    // a member starts at byte `at` (stream offset r.next.stream_out): BGZF blocks are inflated side by side, a large plain member
    // goes to the chunked decoder, anything else to zlib for the rest of the file
    void begin_member(size_t at, Result &r) const {
        Cursor &c = r.next;
        c.bgzf = false;
        c.bgzf_at = 0;
        gzframe::Member m;
        gzframe::Header h;
        const gzframe::Kind kind = gzframe::member_at(data_, size_, at, &m);
        if (kind == gzframe::Kind::BGZF) {
            c.bgzf = true;
            c.bgzf_at = at;
        } else if (kind == gzframe::Kind::OTHER && gzframe::parse_header(data_, size_, at, &h) && (size_ - at >= min_bytes() || at == 0)) {
            if (gpu_ && at > 0) ++r.add.device_handed;  // a plain member behind BGZF ones: the host decoders', like every hand-over
            c.chain_bit = (uint64_t)h.deflate_at * 8;
            c.member_base = c.stream_out;
            c.member_out = 0;
            c.crc = crc32(0L, Z_NULL, 0);
            c.window.clear();
        } else {
            hand_over(r, member_point(at, c.stream_out));
        }
    }

    // BGZF: up to threads x 128 blocks, every thread a run of neighbours
    Result bgzf_round(const Cursor &cur) {
        Result r(cur);
        std::vector<BgzfMember> mem;
        size_t at = cur.bgzf_at;
        gzframe::Kind kind = gzframe::Kind::BGZF;
        while (mem.size() < (size_t)threads_ * 128) {
            gzframe::Member m;
            if ((kind = gzframe::member_at(data_, size_, at, &m)) != gzframe::Kind::BGZF) break;
            mem.push_back({at, m.size, m.isize});
            at += m.size;
        }
        if (mem.empty()) {  // the end of the file, or a member of another kind
            if (kind == gzframe::Kind::NONE) r.end = Result::FINISHED;
            else begin_member(at, r);
            return r;
        }
        const size_t runs = std::min<size_t>(threads_, mem.size());
        std::vector<Piece> pieces(runs);
        std::vector<size_t> first(runs + 1);
        std::vector<size_t> good(runs, 0);  // the members of a run in front of its first bad one
        for (size_t k = 0; k <= runs; ++k) first[k] = mem.size() * k / runs;
        std::atomic<bool> device_failed{false};
        std::atomic<uint64_t> device_ns{0};
        run_parallel(runs, threads_, [&](size_t k) {
            const BgzfMember *m = &mem[first[k]];
            const size_t n = first[k + 1] - first[k];
            size_t total = 0;
            for (size_t i = 0; i < n; ++i) total += m[i].isize;
            Piece &pc = pieces[k];
            pc.bytes = pool_->take();
            if (pc.bytes.size() < total) pc.bytes.resize(total);
            if (gpu_) {
                const auto t0 = std::chrono::steady_clock::now();
                if (!device_run(m, n, pc.bytes.data(), &good[k])) device_failed = true;
                device_ns += (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count();
            } else {
                good[k] = zlib_run(m, n, pc.bytes.data());
            }
            for (size_t i = 0; i < good[k]; ++i) pc.n += m[i].isize;
        });
        if (device_failed) good.assign(runs, 0);  // the device inflater could not run: zlib reads on alone from the first run
        r.add.device_ns = device_ns;
        r.add.rounds = 1;
        Cursor &c = r.next;
        for (size_t k = 0; k < runs; ++k) {
            if (good[k] > 0) {  // the members in front of a bad one are a piece like any other
                if (c.stream_out > 0) r.batch.points.push_back(member_point(mem[first[k]].at, c.stream_out));
                c.stream_out += pieces[k].n;
                r.add.parallel_bytes += pieces[k].n;
                if (gpu_) r.add.device_members += good[k];
                if (pieces[k].n > 0) r.batch.pieces.push_back(std::move(pieces[k]));
            }
            const size_t bad = first[k] + good[k];
            if (bad < first[k + 1]) {  // zlib reads on from the bad member, alone, and says what is wrong with it
                if (gpu_) r.add.device_handed += mem.size() - bad - 1;  // (hand_over counts the bad member itself)
                c.bgzf = false;
                hand_over(r, member_point(mem[bad].at, c.stream_out));
                return r;
            }
        }
        c.bgzf_at = at;
        return r;
    }

    // one round of a plain member: up to `threads` chunks searched, decoded, chained, resolved
    Result chunk_round(const Cursor &cur, unsigned round_no) {
        Result r(cur);
        r.add.rounds = 1;
        static const bool timing = getenv("FLX_CLI_PINFLATE_TIMING") != nullptr;
        auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
        const double t0 = now();
        const uint64_t data_end = (uint64_t)(size_ - 8) * 8;  // the trailer is not deflate data
        const size_t cb = chunk_bytes();
        const uint64_t base_byte = cur.chain_bit >> 3;
        const uint64_t left_bytes = (data_end >> 3) > base_byte ? (data_end >> 3) - base_byte : 0;
        const size_t n = (size_t)std::max<uint64_t>(1, std::min<uint64_t>(threads_, (left_bytes + cb - 1) / cb));
        std::vector<Chunk> ch(n);
        const uint64_t round_end = std::min<uint64_t>(data_end, (base_byte + (uint64_t)n * cb) * 8);
        for (size_t i = 0; i < n; ++i) {
            ch[i].begin = i == 0 ? cur.chain_bit : std::min<uint64_t>(round_end, (base_byte + (uint64_t)i * cb) * 8);
            ch[i].end = i + 1 < n ? std::min<uint64_t>(round_end, (base_byte + (uint64_t)(i + 1) * cb) * 8) : round_end;
        }
        ch[0].found = true;
        ch[0].start = cur.chain_bit;
        const size_t limit = std::max<size_t>(cb * 24, (size_t)1 << 20);  // a text compresses 3-5x; beyond 24x zlib does it alone
        run_parallel(n, threads_, [&](size_t i) {
            Decoder &d = decoders_[i];
            d.in.init(data_, size_);
            if (i == 0) return;
            d.limit = (size_t)1 << 22;
            if (d.out.size() < ((size_t)1 << 16)) d.out.resize((size_t)1 << 16);
            ch[i].found = ch[i].begin < ch[i].end && find_block_start(d, ch[i].begin, ch[i].end, &ch[i].start);
        });
        const double t1 = now();
        run_parallel(n, threads_, [&](size_t i) {
            Chunk &c = ch[i];
            if (!c.found) return;
            Decoder &d = decoders_[i];
            d.limit = limit;
            d.n = 0;
            d.in.seek(c.start);
            size_t j = i + 1;
            size_t scanned = 0, clean_from = 0;  // clean_from: one past the last marker among the symbols scanned
            uint64_t tail_from = 0;
            bool tail = false;
            for (;;) {
                bool fin = false;
                const Status st = d.any_block(&fin, false);
                if (st != OK) { c.status = st; break; }
                if (fin) { c.status = OK; c.final_block = true; c.stop = (d.in.pos() + 7) & ~7ull; break; }
                const uint64_t p = d.in.pos();
                if (chain_stop(c, p, ch, &j, round_end)) break;
                if (zlib_tails_) {  // once 32 KiB without a marker are behind us, the rest does not depend on the unknown window: zlib's
                    for (const uint16_t *s = d.out.data(); scanned < d.n; ++scanned)
                        if (s[scanned] >= 256) clean_from = scanned + 1;
                    if (d.n - clean_from >= 32768) { tail = true; tail_from = p; break; }
                }
            }
            c.n_sym = c.n = d.n;
            c.sym.swap(d.out);  // (handed back below)
            c.bytes = pool_->take();
            if (tail) zlib_tail(c, tail_from, ch, j, round_end, limit);
            else if (c.bytes.size() < c.n) c.bytes.resize(c.n);
        });
        const double t2 = now();
        // the chain from chunk 0; windows one after the other
        std::vector<size_t> chain;
        size_t i = 0;
        size_t broken = (size_t)-1;
        uint64_t out = cur.member_out;
        std::string window = cur.window;
        for (;;) {
            Chunk &c = ch[i];
            c.out = out;
            c.window = window;
            if (c.status != OK) { broken = i; break; }
            if (!next_window(c, &window)) { broken = i; break; }
            chain.push_back(i);
            out += c.n;
            if (c.final_block || c.arrived < 0) break;
            i = (size_t)c.arrived;
        }
        for (size_t k = 0; k < n; ++k) r.add.dropped_chunks += ch[k].found && std::find(chain.begin(), chain.end(), k) == chain.end() && k != broken;
        // markers -> bytes, CRC-32 per chunk
        const double t3 = now();
        run_parallel(chain.size(), threads_, [&](size_t k) {
            Chunk &c = ch[chain[k]];
            char *dst = c.bytes.data();
            const uint16_t *s = c.sym.data();
            const size_t wn = c.window.size();
            const unsigned char *w = (const unsigned char *)c.window.data();
            for (size_t q = 0; q < c.n_sym; ++q) {
                const unsigned v = s[q];
                if (v < 256) { dst[q] = (char)v; continue; }
                const size_t back = 32768 - (v - 256);  // bytes in front of the chunk
                if (back > wn) { c.bad_marker = true; dst[q] = 0; continue; }
                dst[q] = (char)w[wn - back];
            }
            uLong crc = crc32(0L, Z_NULL, 0);
            for (size_t at = 0; at < c.n; at += (size_t)1 << 30)
                crc = crc32(crc, (const Bytef *)dst + at, (uInt)std::min<size_t>(c.n - at, (size_t)1 << 30));
            c.crc = crc;
        });
        if (timing) {
            size_t tail = 0, all = 0;
            for (size_t k : chain) { tail += ch[k].n - ch[k].n_sym; all += ch[k].n; }
            fprintf(stderr, "[pinflate] round %u: search %.3f  decode %.3f  chain %.3f  resolve+crc %.3f s, %zu of %zu chunks chained, %zu bytes (%zu by zlib)\n",
                    round_no, t1 - t0, t2 - t1, t3 - t2, now() - t3, chain.size(), n, all, tail);
        }
        // the symbol buffers go back to the decoders
        for (size_t k = 0; k < n; ++k)
            if (ch[k].sym.size() > decoders_[k].out.size()) decoders_[k].out.swap(ch[k].sym);
        size_t good = chain.size();
        for (size_t k = 0; k < chain.size(); ++k)
            if (ch[chain[k]].bad_marker) { good = k; break; }  // a distance too far back: zlib will say so
        if (good < chain.size()) {
            broken = chain[good];
            chain.resize(good);
        }
        Cursor &nc = r.next;
        for (size_t k = 0; k < chain.size(); ++k) {
            Chunk &c = ch[chain[k]];
            nc.crc = crc32_combine(nc.crc, c.crc, (z_off_t)c.n);
            if (nc.member_base + c.out > 0) r.batch.points.push_back(point_at(nc, c.start, c.out, c.window));
            r.add.parallel_bytes += c.n;
            nc.stream_out += c.n;
            r.add.zlib_tail_bytes += c.n - c.n_sym;
            if (c.n > 0) {
                Piece pc;
                pc.bytes = std::move(c.bytes);
                pc.n = c.n;
                r.batch.pieces.push_back(std::move(pc));
            }
        }
        if (broken != (size_t)-1) {  // zlib continues from the start of the chunk that did not work out
            const Chunk &c = ch[broken];
            hand_over(r, point_at(nc, c.start, c.out, c.window, true));
            return r;
        }
        const Chunk &last = ch[chain.back()];
        nc.member_out = out;
        nc.window = window;
        nc.chain_bit = last.stop;
        if (last.final_block) finish_member(last.stop, r);
        return r;
    }

private:
    struct BgzfMember { size_t at, size; uint32_t isize; };
    struct Chunk {
        uint64_t begin = 0, end = 0;  // the bits this chunk searches
        uint64_t start = 0;           // where its decoding began
        bool found = false;
        Status status = FAIL;
        uint64_t stop = 0;   // block boundary it stopped at
        int arrived = -1;    // the chunk whose start that is (-1: the end of the round)
        bool final_block = false;
        std::vector<uint16_t> sym;  // the head of the chunk as symbols (markers possible) ...
        size_t n_sym = 0;
        std::vector<char> bytes;    // ... and all of it as bytes: [0, n_sym) filled in once the window is known, the rest by zlib
        size_t n = 0;
        uint64_t out = 0;    // member offset of its first byte
        uLong crc = 0;
        bool bad_marker = false;
        std::string window;  // the (up to) 32 KiB in front of it
    };

    // The two ways to inflate the n members of a run into `out`, one behind the other: how many of them, from the front, came out
    // right.  zlib (which checks each member's CRC-32 and size) says all or none.
    size_t zlib_run(const BgzfMember *m, size_t n, char *out) const {
        z_stream z;
        memset(&z, 0, sizeof z);
        if (inflateInit2(&z, 31) != Z_OK) return 0;
        bool ok = true;
        for (size_t k = 0; k < n && ok; ++k) {
            z.next_in = (Bytef *)data_ + m[k].at; z.avail_in = (uInt)m[k].size;
            z.next_out = (Bytef *)out; z.avail_out = (uInt)m[k].isize;
            ok = inflate(&z, Z_FINISH) == Z_STREAM_END && z.avail_in == 0 && z.avail_out == 0;
            out += m[k].isize;
            ok = inflateReset(&z) == Z_OK && ok;
        }
        inflateEnd(&z);
        return ok ? n : 0;
    }
    // the device stops counting at the first member it does not call ok; false: it could not run at all
    bool device_run(const BgzfMember *m, size_t n, char *out, size_t *good) const {
        std::vector<uint64_t> in_off(n + 1), out_off(n + 1);
        in_off[0] = 0;
        out_off[0] = 0;
        for (size_t k = 0; k < n; ++k) {
            in_off[k + 1] = in_off[k] + m[k].size;
            out_off[k + 1] = out_off[k] + m[k].isize;
        }
        uint64_t first_bad = 0;
        if (flx_bgzf_inflate(gpu_, data_ + m[0].at, in_off.data(), out_off.data(), n, out, &first_bad) != FLX_OK) return false;
        *good = (size_t)first_bad;
        return true;
    }

    // The chain's stop rule for chunk c at block boundary p: later chunks' starts it ran past were no block boundaries (*j skips
    // them); it stops at a start it meets, and at the first boundary behind the round.
    static bool chain_stop(Chunk &c, uint64_t p, const std::vector<Chunk> &ch, size_t *j, uint64_t round_end) {
        while (*j < ch.size() && (!ch[*j].found || ch[*j].start < p)) ++*j;
        if (*j < ch.size() && ch[*j].start == p) c.arrived = (int)*j;
        else if (p < round_end) return false;
        c.status = OK;
        c.stop = p;
        return true;
    }

    // Chunk c from block boundary `bit` on with zlib: the 32 KiB in front of it are known bytes (the last 32768 symbols are literals).
    // Stops like the marker decoder (chain_stop), or at the end of the member.
    void zlib_tail(Chunk &c, uint64_t bit, const std::vector<Chunk> &ch, size_t j, uint64_t round_end, size_t limit) const {
        char dict[32768];
        for (size_t q = 0; q < 32768; ++q) dict[q] = (char)c.sym[c.n_sym - 32768 + q];
        uint64_t in_pos = (bit + 7) >> 3;
        size_t have = c.n_sym;
        c.status = FAIL;
        z_stream z;
        if (!inflate_resume(&z, data_, in_pos, (int)((8 - (bit & 7)) & 7), dict, 32768)) return;
        for (;;) {
            if (c.bytes.size() < have + ((size_t)1 << 16)) {
                if (have > limit) { c.status = LIMIT; break; }
                c.bytes.resize(std::max<size_t>(c.bytes.size() * 2, have + ((size_t)1 << 20)));
            }
            const size_t out_room = std::min<size_t>(c.bytes.size() - have, (size_t)1 << 30);
            const size_t in_room = (size_t)std::min<uint64_t>(size_ - in_pos, (uint64_t)1 << 30);
            z.next_out = (Bytef *)c.bytes.data() + have; z.avail_out = (uInt)out_room;
            z.next_in = (Bytef *)data_ + in_pos; z.avail_in = (uInt)in_room;
            const int ret = inflate(&z, Z_BLOCK);
            const size_t got = out_room - z.avail_out;
            have += got;
            in_pos += in_room - z.avail_in;
            if (ret == Z_STREAM_END) { c.status = OK; c.final_block = true; c.stop = in_pos * 8; break; }
            if (ret != Z_OK && ret != Z_BUF_ERROR) break;
            if (got == 0 && in_room == z.avail_in && (ret == Z_BUF_ERROR || in_pos >= size_)) break;  // truncated
            if ((z.data_type & 128) && !(z.data_type & 64) &&  // at a block boundary, not in the last block
                chain_stop(c, in_pos * 8 - (uint64_t)(z.data_type & 7), ch, &j, round_end)) break;
        }
        inflateEnd(&z);
        c.n = have;
    }

    // the 32 KiB behind chunk c from the 32 KiB in front of it, its symbols and its bytes; false: a marker points in front of the data
    static bool next_window(const Chunk &c, std::string *window) {
        const std::string &w = c.window;
        const size_t keep = 32768;
        const size_t n_tail = c.n - c.n_sym;                       // bytes zlib wrote
        const size_t from_tail = std::min(n_tail, keep);
        const size_t from_sym = std::min(c.n_sym, keep - from_tail);
        const size_t from_w = std::min(w.size(), keep - from_tail - from_sym);
        std::string nw;
        nw.reserve(keep);
        nw.append(w, w.size() - from_w, from_w);
        for (size_t q = c.n_sym - from_sym; q < c.n_sym; ++q) {
            const unsigned v = c.sym[q];
            if (v < 256) { nw.push_back((char)v); continue; }
            const size_t back = 32768 - (v - 256);
            if (back > w.size()) return false;
            nw.push_back(w[w.size() - back]);
        }
        nw.append(c.bytes.data() + c.n - from_tail, from_tail);
        window->swap(nw);
        return true;
    }

    // the member of r.next ended at end_bit: its trailer, and what follows
    void finish_member(uint64_t end_bit, Result &r) const {
        const Cursor &c = r.next;
        size_t next = 0;
        const gzframe::End e = gzframe::member_end(data_, size_, (size_t)((end_bit + 7) >> 3), (uint32_t)c.crc, (uint32_t)c.member_out, &next);
        r.end = Result::FINISHED;  // (a trailer that is cut off: to gzread the end of the file, everything decoded is delivered)
        if (e == gzframe::End::MISMATCH) {  // zlib: "incorrect data check" / "incorrect length check"
            r.end = Result::ERROR;
            r.deliverable = gzread_delivered_before_error(c.member_base, c.member_out, false);
        } else if (e == gzframe::End::MEMBER_FOLLOWS) {  // like gzread: members follow each other
            r.end = Result::GO_ON;
            begin_member(next, r);
        }
    }

    const unsigned char *data_ = nullptr;
    size_t size_ = 0;
    unsigned threads_ = 1;
    bool zlib_tails_ = true;
    flx_bgzf *gpu_ = nullptr;  // the device inflater of BGZF members (null: the zlib workers)
    BufferPool *pool_ = nullptr;
    std::vector<Decoder> decoders_;
};

}  // namespace pinflate
