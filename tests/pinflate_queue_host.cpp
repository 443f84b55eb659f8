// pinflate_queue_host.cpp — the hand-off queue of the parallel gzip reader (filtlong_amd/cli/pinflate_queue.h) on its own, and the
// reader's shutdown through it.  One case per run: pinflate_queue_host CASE; prints "ok CASE" or says what went wrong (exit 1).  A
// case that hangs is ended by the caller's time limit (tests/test_pinflate_layers_host.py).
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <string>
#include <thread>
#include "pinflate.h"  // -I filtlong_amd/cli

struct flx_bgzf { int unused; };
extern "C" int flx_bgzf_inflate(flx_bgzf *, const void *, const uint64_t *, const uint64_t *, uint64_t, void *, uint64_t *) { return FLX_ERR_INVALID; }

using pinflate::Batch;
using pinflate::Handoff;
using pinflate::Piece;

static const size_t kAhead = 1000;
static int fail(const char *what) { printf("FAILED: %s\n", what); return 1; }
static void settle() { std::this_thread::sleep_for(std::chrono::milliseconds(30)); }  // (lets the other thread reach its wait)

static Batch batch_of(size_t bytes, uint64_t *offset) {  // one piece whose bytes count on from *offset, and a point at its start
    Batch b;
    GzPoint pt;
    pt.out = *offset;
    b.points.push_back(pt);
    if (bytes > 0) {
        Piece pc;
        pc.bytes.resize(bytes);
        for (size_t i = 0; i < bytes; ++i) pc.bytes[i] = (char)((*offset + i) * 31 >> 3);
        pc.n = bytes;
        b.pieces.push_back(std::move(pc));
    }
    *offset += bytes;
    return b;
}

// batches whose sizes straddle the limit, a reader that drains at once for a while and then lags: every byte and point in order,
// "finished" with the last batch and not before, and never more in the queue than the limit and one batch
static int flow() {
    static const size_t sizes[] = {0, 1, kAhead - 1, kAhead, kAhead + 1, 3 * kAhead, 7, 0, 2 * kAhead + 1};
    const size_t n_sizes = sizeof sizes / sizeof *sizes, n_batches = 400;
    Handoff q;
    q.reset(kAhead);
    uint64_t total = 0;
    for (size_t k = 0; k < n_batches; ++k) total += sizes[k % n_sizes];
    std::thread producer([&] {
        uint64_t offset = 0;
        for (size_t k = 0; k < n_batches; ++k) {
            Batch b = batch_of(sizes[k % n_sizes], &offset);
            if (!q.publish(b, k + 1 == n_batches)) return;
            if (!b.pieces.empty() || !b.points.empty()) return;  // (publish empties what it takes)
        }
    });
    uint64_t seen = 0, points = 0, takes = 0;
    bool finished = false, bad = false;
    while (!finished) {
        Batch got;
        finished = q.take(&got);
        size_t bytes = 0;
        for (const Piece &pc : got.pieces) {
            for (size_t i = 0; i < pc.n; ++i) bad = bad || pc.bytes[i] != (char)((seen + i) * 31 >> 3);
            seen += pc.n;
            bytes += pc.n;
        }
        for (const GzPoint &pt : got.points) { bad = bad || pt.out > seen; ++points; }
        bad = bad || bytes > kAhead + 3 * kAhead;
        bad = bad || (got.pieces.empty() && !finished);  // take() returns with a piece, or at the end
        if ((++takes / 16) % 2) std::this_thread::sleep_for(std::chrono::microseconds(200));  // lag for 16 takes, drain for 16
    }
    producer.join();
    if (bad) return fail("order, content or the bound on what is queued");
    if (seen != total || points != n_batches) return fail("bytes or points lost");
    return 0;
}

static int stop_while_producer_waits() {
    Handoff q;
    q.reset(kAhead);
    std::atomic<int> returned{-1};
    std::thread producer([&] {
        uint64_t offset = 0;
        Batch b = batch_of(5 * kAhead, &offset);
        returned = q.publish(b, false) ? 1 : 0;  // more than the limit and nobody reads: waits for room
    });
    settle();
    if (returned != -1) return producer.join(), fail("publish did not wait for room");
    q.stop();
    producer.join();
    if (returned != 0) return fail("publish did not say that the stream was given up");
    Batch got;
    if (!q.take(&got)) return fail("take after stop does not say finished");
    Batch more;
    uint64_t offset = 0;
    more = batch_of(10, &offset);
    if (q.publish(more, false)) return fail("publish after stop");
    return 0;
}

static int stop_while_reader_waits() {
    Handoff q;
    q.reset(kAhead);
    std::atomic<int> returned{-1};
    Batch got;
    std::thread reader([&] { returned = q.take(&got) ? 1 : 0; });
    settle();
    if (returned != -1) return reader.join(), fail("take did not wait for data");
    q.stop();
    reader.join();
    if (returned != 1 || !got.pieces.empty()) return fail("take after stop");
    return 0;
}

static int unread_at_destruction() {
    {
        Handoff q;
        q.reset(kAhead);
        uint64_t offset = 0;
        Batch b = batch_of(kAhead / 2, &offset);
        if (!q.publish(b, false)) return fail("publish below the limit");
        b = batch_of(kAhead, &offset);
        if (!q.publish(b, true)) return fail("the last publish");
    }
    // the reader itself: 6 MB of text as one gzip member, the producer allowed 1 MiB ahead, one small read, then the destructor
    // while the producer waits for room
    std::string text;
    for (unsigned i = 0; text.size() < (6u << 20); ++i) {
        char line[128];
        snprintf(line, sizeof line, "@read_%u ch=%u\nACGTTGCA%08xGATTACA\n+\nIIIIHHHHGGGGFFFFEEEEDDD\n", i, i % 512, i * 2654435761u);
        text += line;
    }
    std::vector<unsigned char> gz(compressBound((uLong)text.size()) + 64);
    z_stream z;
    memset(&z, 0, sizeof z);
    if (deflateInit2(&z, 6, Z_DEFLATED, 31, 8, Z_DEFAULT_STRATEGY) != Z_OK) return fail("deflateInit2");
    z.next_in = (Bytef *)text.data(); z.avail_in = (uInt)text.size();
    z.next_out = gz.data(); z.avail_out = (uInt)gz.size();
    if (deflate(&z, Z_FINISH) != Z_STREAM_END) return fail("deflate");
    gz.resize(z.total_out);
    deflateEnd(&z);
    setenv("FLX_CLI_PINFLATE_MIN", "1", 1);
    setenv("FLX_CLI_PINFLATE_CHUNK", "20000", 1);
    setenv("FLX_CLI_PINFLATE_AHEAD_MB", "1", 1);
    for (int reads = 0; reads < 3; ++reads) {
        ParallelInflate in;
        if (!in.open(gz.data(), gz.size(), true, 4)) return fail("open");
        std::vector<char> buf(32768 + 1000);
        for (int k = 0; k < reads; ++k)
            if (in.read(buf.data() + 32768, 1000) != 1000 || memcmp(buf.data() + 32768, text.data() + 1000 * k, 1000) != 0) return fail("read");
        if (reads == 2) settle();  // (once with the producer surely waiting)
        if (in.rounds() == 0 && reads > 0) return fail("the reader did not go through the rounds");
    }
    return 0;
}

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    const std::string c = argv[1];
    const int rc = c == "flow" ? flow() : c == "stop_while_producer_waits" ? stop_while_producer_waits() :
                   c == "stop_while_reader_waits" ? stop_while_reader_waits() : c == "unread_at_destruction" ? unread_at_destruction() : 2;
    if (rc == 0) printf("ok %s\n", argv[1]);
    return rc;
}
