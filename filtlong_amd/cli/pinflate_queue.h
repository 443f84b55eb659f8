// pinflate_queue.h — the hand-off between the two threads of the parallel gzip reader (pinflate.h): the producer publishes what a
// round decoded and waits while it is more than `max_ahead` bytes in front of the reader; the reader takes everything there is.
// All that the two threads share lives in this file: the queue behind one mutex, the pool of byte buffers behind another.
#pragma once
#include <condition_variable>
#include <deque>
#include <mutex>
#include <vector>

#include "inflate_stream.h"

namespace pinflate {

struct Piece {  // decoded bytes, in stream order
    std::vector<char> bytes;
    size_t n = 0, pos = 0;  // valid bytes, of which read
};
struct Batch {  // what one round adds to the stream: its pieces and the access points at their boundaries
    std::deque<Piece> pieces;
    std::deque<GzPoint> points;
};

class Handoff {
public:
    // (no thread is inside: before the producer starts)
    void reset(size_t max_ahead) {
        q_ = Batch();
        queued_bytes_ = 0;
        max_ahead_ = max_ahead;
        finished_ = stop_ = false;
    }
    // Producer: appends b (emptied); last: nothing follows.  Returns when the reader is at most max_ahead bytes behind, or at once
    // after `last` or stop().  false: stop() was called, the producer leaves.
    bool publish(Batch &b, bool last) {
        std::unique_lock<std::mutex> lk(mu_);
        for (Piece &pc : b.pieces) { queued_bytes_ += pc.n; q_.pieces.push_back(std::move(pc)); }
        for (GzPoint &pt : b.points) q_.points.push_back(std::move(pt));
        b = Batch();
        if (last) finished_ = true;
        cv_.notify_all();
        cv_.wait(lk, [&] { return queued_bytes_ <= max_ahead_ || finished_; });
        return !stop_;
    }
    // Reader: everything published so far, appended to *to; waits until there is a piece or the producer has finished.  true: finished
    // (with what this call took, that was all).
    bool take(Batch *to) {
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [&] { return !q_.pieces.empty() || finished_; });
        for (Piece &pc : q_.pieces) to->pieces.push_back(std::move(pc));
        for (GzPoint &pt : q_.points) to->points.push_back(std::move(pt));
        q_ = Batch();
        queued_bytes_ = 0;
        cv_.notify_all();
        return finished_;
    }
    // Anyone: the stream is given up.  Whoever waits returns, publish() says false from now on, take() says finished.
    void stop() {
        std::lock_guard<std::mutex> g(mu_);
        stop_ = finished_ = true;
        cv_.notify_all();
    }

private:
    std::mutex mu_;
    std::condition_variable cv_;
    Batch q_;
    size_t queued_bytes_ = 0, max_ahead_ = (size_t)256 << 20;
    bool finished_ = false, stop_ = false;
};

// The other thing both threads touch: byte buffers to use again.  The producer's workers take, the reader gives back what it has read.
class BufferPool {
public:
    std::vector<char> take() {
        std::lock_guard<std::mutex> g(mu_);
        if (free_.empty()) return std::vector<char>();
        std::vector<char> v = std::move(free_.back());
        free_.pop_back();
        return v;
    }
    void give(std::vector<char> &&v, size_t keep_at_most) {
        std::lock_guard<std::mutex> g(mu_);
        if (free_.size() < keep_at_most) free_.push_back(std::move(v));
    }

private:
    std::mutex mu_;
    std::vector<std::vector<char>> free_;
};

}  // namespace pinflate
