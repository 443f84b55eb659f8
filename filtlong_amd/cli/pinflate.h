// pinflate.h — pass 1 of a compressed input on all host threads, behind the interface of the serial reader.
//
// The reference reads a gzip input through zlib's gzread, one thread (src/main.cpp:70 via src/kseq.h:87-110); pass 1 of the
// streamed reader here did the same (inflate_stream.h) and was the longest stage of a compressed run.  The layers, bottom up:
//   ../csrc/gzip_framing.h  where a member begins and ends, which members are BGZF blocks (shared with flx_bgzf_index);
//   deflate_markers.h       the RFC 1951 decoder that starts without its window;
//   pinflate_rounds.h       a round: from a position in the file to the bytes decoded from there and the next position;
//   pinflate_queue.h        the bounded hand-off between the thread that makes rounds and the one that reads;
//   this file               ParallelInflate: a producer thread commits round after round, read() copies out what it is given, and
//                           zlib (InflateStream) takes over wherever the rounds end without having reached the end of the file.
#pragma once
#include "pinflate_rounds.h"

// Same interface as InflateStream (which it falls back to and hands over to): sequential reads of the uncompressed bytes.
class ParallelInflate {
public:
    static size_t min_bytes() { return pinflate::min_bytes(); }
    static unsigned default_threads(unsigned host_threads) {  // decoding scales further than the host's memory-bound stages
        if (const char *e = getenv("FLX_CLI_INFLATE_THREADS")) return (unsigned)std::max(1, atoi(e));
        if (getenv("FLX_CLI_THREADS")) return host_threads;
        return std::max(host_threads, std::min(32u, std::thread::hardware_concurrency()));
    }
    static size_t chunk_bytes() { return pinflate::chunk_bytes(); }

    ParallelInflate() = default;
    ParallelInflate(const ParallelInflate &) = delete;
    ParallelInflate &operator=(const ParallelInflate &) = delete;
    ~ParallelInflate() { shutdown(); }

    // BGZF members go through this device inflater instead of the zlib workers (null, the default: nothing changes).  Set before
    // open().  What the device does not call ok goes to zlib, member by member, exactly as a failing run of the workers does.
    void set_device(flx_bgzf *z) { gpu_ = z; }
    uint64_t device_members() const { return device_members_; }

    bool open(const unsigned char *data, size_t size, bool gz, unsigned threads) {
        shutdown();
        data_ = data; size_ = size; threads_ = std::max(1u, threads);
        serial_mode_ = true; done_ = false; error_ = false;
        delivered_ = 0; last_point_out_ = 0; got_ = pinflate::Batch();
        ended_ = pinflate::Result::FINISHED; deliverable_ = 0;
        parallel_bytes_ = 0; zlib_tail_bytes_ = 0; rounds_ = 0; dropped_chunks_ = 0;
        device_members_ = 0; device_handed_ = 0; device_ns_ = 0;
        const char *off = getenv("FLX_CLI_PINFLATE");  // 0: zlib only; "nozlib": every chunk to its end with the marker decoder (tests)
        size_t max_ahead = (size_t)256 << 20;
        if (const char *e = getenv("FLX_CLI_PINFLATE_AHEAD_MB")) max_ahead = (size_t)std::max(1, atoi(e)) << 20;
        if (gz && threads_ >= 2 && size >= min_bytes() && !(off && off[0] == '0')) {
            rounds_maker_.init(data, size, threads_, gpu_, !(off && strcmp(off, "nozlib") == 0), &pool_);
            pinflate::Result first;
            rounds_maker_.begin_member(0, first);
            commit(first);
            if (first.end != pinflate::Result::GO_ON) { device_line(); return take_over(); }  // nothing for the rounds: zlib from the first byte
            serial_mode_ = false;
            handoff_.reset(max_ahead);
            producer_ = std::thread([this, from = std::move(first.next)] { produce(from); });  // decodes ahead of read()
            return true;
        }
        return serial_.open(data, size, gz);
    }
    bool eof() const { return got_.pieces.empty() && (serial_mode_ ? serial_.eof() : done_); }
    bool error() const { return error_ || (serial_mode_ && serial_.error()); }
    // after error(): how many bytes of the stream zlib's gzread would have handed to the reference's parser before its error
    // state (inflate_stream.h: gzread_delivered_before_error) — up to 32 KiB fewer than read() has produced.  A stream that is
    // merely TRUNCATED is no error: everything decodable comes out, then eof(), like gzread.
    uint64_t deliverable() const { return serial_mode_ && serial_.error() ? serial_.deliverable() : deliverable_; }
    uint64_t total_out() const { return delivered_; }
    // diagnostics: bytes that came out of the rounds (of those: from zlib running behind the marker decoder), rounds, chunks whose
    // work was dropped
    uint64_t parallel_bytes() const { return parallel_bytes_; }
    uint64_t zlib_tail_bytes() const { return zlib_tail_bytes_; }
    unsigned rounds() const { return rounds_; }
    unsigned dropped_chunks() const { return dropped_chunks_; }

    // like InflateStream::read: up to cap bytes to dst (the caller keeps the previous 32 KiB in front of dst + n); access points at
    // least `span` output bytes apart are appended to *points
    size_t read(char *dst, size_t cap, std::vector<GzPoint> *points = nullptr, uint64_t span = 0) {
        std::deque<pinflate::Piece> &queue = got_.pieces;
        std::deque<GzPoint> &pending = got_.points;
        size_t produced = 0;
        while (produced < cap && !error_) {
            if (queue.empty() && !serial_mode_ && !done_) {  // what the producer has ready; wait for it if that is nothing
                if (handoff_.take(&got_) && queue.empty()) {  // the producer has left: the end, an error, or zlib's turn
                    if (producer_.joinable()) producer_.join();
                    if (ended_ == pinflate::Result::ERROR) error_ = true;
                    else if (ended_ == pinflate::Result::HAND_OVER) take_over();
                    else done_ = true;
                }
                continue;
            }
            if (!queue.empty()) {  // whole chunks to their places on all threads
                struct Copy { const char *from; char *to; size_t n; };
                std::vector<Copy> plan;
                size_t at = produced;
                for (const pinflate::Piece &pc : queue) {
                    const size_t m = std::min(cap - at, pc.n - pc.pos);
                    if (m == 0) break;
                    for (size_t o = 0; o < m; o += (size_t)4 << 20)
                        plan.push_back({pc.bytes.data() + pc.pos + o, dst + at + o, std::min<size_t>(m - o, (size_t)4 << 20)});
                    at += m;
                    if (m < pc.n - pc.pos) break;
                }
                pinflate::run_parallel(plan.size(), threads_, [&](size_t k) { memcpy(plan[k].to, plan[k].from, plan[k].n); });
                size_t left = at - produced;
                produced = at;
                delivered_ += left;
                while (left > 0) {
                    pinflate::Piece &pc = queue.front();
                    const size_t m = std::min(left, pc.n - pc.pos);
                    pc.pos += m;
                    left -= m;
                    if (pc.pos >= pc.n) {
                        pool_.give(std::move(pc.bytes), 3 * (size_t)threads_);
                        queue.pop_front();
                    }
                }
                while (!pending.empty() && pending.front().out <= delivered_) {
                    if (points && pending.front().out - last_point_out_ >= span) {
                        last_point_out_ = pending.front().out;
                        points->push_back(std::move(pending.front()));
                    }
                    pending.pop_front();
                }
                continue;
            }
            if (serial_mode_) {
                const size_t m = serial_.read(dst + produced, cap - produced, points, span);
                produced += m; delivered_ += m;
                break;  // (less than asked for only at the end or on an error)
            }
            break;  // done_
        }
        return produced;
    }

private:
    // The producer thread: round after round from `cur`, each committed whole and published to the reader.  A round that cannot get
    // its memory (std::bad_alloc out of a vector, here or in a worker) must not end the process: it has changed nothing, and zlib
    // reads on alone from the cursor it began at.
    void produce(pinflate::Cursor cur) {
        for (;;) {
            pinflate::Result r;
            try {
                r = cur.bgzf ? rounds_maker_.bgzf_round(cur) : rounds_maker_.chunk_round(cur, rounds_ + 1);
            } catch (...) {
                r = pinflate::Result();
                rounds_maker_.hand_over(r, rounds_maker_.point_of(cur));
            }
            commit(r);
            cur = std::move(r.next);
            const bool last = r.end != pinflate::Result::GO_ON;
            const bool go_on = handoff_.publish(r.batch, last);
            if (last) device_line();
            if (last || !go_on) return;
        }
    }
    // what a round (or the first look at the file) says about the stream; the reader looks at the end state once the producer has left
    void commit(const pinflate::Result &r) {
        parallel_bytes_ += r.add.parallel_bytes; zlib_tail_bytes_ += r.add.zlib_tail_bytes;
        rounds_ += r.add.rounds; dropped_chunks_ += r.add.dropped_chunks;
        device_members_ += r.add.device_members; device_handed_ += r.add.device_handed; device_ns_ += r.add.device_ns;
        ended_ = r.end;
        deliverable_ = r.deliverable;
        handover_ = r.handover;
    }
    // FLX_CLI_PINFLATE_TIMING with a device inflater: what it did, once, when the producer has finished
    void device_line() const {
        if (!gpu_ || !getenv("FLX_CLI_PINFLATE_TIMING")) return;
        fprintf(stderr, "[pinflate] device: %llu members inflated on the device, %llu handed to zlib, %.3f ms in flx_bgzf_inflate\n",
                (unsigned long long)device_members_.load(), (unsigned long long)device_handed_.load(), device_ns_.load() * 1e-6);
    }
    // reader: the serial stream takes over where the producer stopped
    bool take_over() {
        serial_mode_ = true;
        const GzPoint &pt = handover_;
        const bool ok = (pt.in == 0 && !pt.raw) ? serial_.open(data_, size_, true) : serial_.open_at(data_, size_, true, pt);
        if (!ok) error_ = true;
        return ok;
    }
    void shutdown() {
        if (!producer_.joinable()) return;
        handoff_.stop();
        producer_.join();
    }

    // set by open()
    const unsigned char *data_ = nullptr;
    size_t size_ = 0;
    unsigned threads_ = 1;
    flx_bgzf *gpu_ = nullptr;
    // the reading thread's
    InflateStream serial_;
    bool serial_mode_ = true, done_ = false, error_ = false;
    uint64_t delivered_ = 0;  // bytes handed to the caller
    uint64_t last_point_out_ = 0;
    pinflate::Batch got_;     // taken from the producer and not yet read
    std::thread producer_;
    // the producer's (open()'s before the thread starts); the reader looks after it has joined the thread
    pinflate::Rounds rounds_maker_;
    pinflate::Result::End ended_ = pinflate::Result::FINISHED;
    uint64_t deliverable_ = 0;  // with ERROR: the bytes gzread would have delivered
    GzPoint handover_;          // with HAND_OVER
    // written by the producer, read by anyone (diagnostics)
    std::atomic<uint64_t> parallel_bytes_{0}, zlib_tail_bytes_{0};
    std::atomic<unsigned> rounds_{0}, dropped_chunks_{0};
    std::atomic<uint64_t> device_members_{0}, device_handed_{0}, device_ns_{0};
    // shared, each behind its own lock
    pinflate::BufferPool pool_;
    pinflate::Handoff handoff_;
};
