// pinflate_layers_host.cpp — everything a caller of ParallelInflate (filtlong_amd/cli/pinflate.h) can see of one file, as text: a
// digest of the bytes, every access point field by field, the end state and the counters.  Rounds and points depend on the thread
// count, FLX_CLI_PINFLATE_CHUNK and the span, not on timing, so two builds of the reader that print the same lines for the same
// arguments behave the same (tools/pinflate_trace_compare.py runs two builds over a corpus).
//   pinflate_layers_host FILE THREADS READ_BYTES SPAN [device]
// device: BGZF members go through a flx_bgzf_inflate made of the host walk of bgzf_inflate_member.h, as in pinflate_device_host.cpp.
// Uses nothing but the reader's public interface.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>
struct uint4 { unsigned x, y, z, w; };
#include "bgzf_inflate_member.h"  // -I filtlong_amd/csrc
#include "pinflate.h"             // -I filtlong_amd/cli

struct flx_bgzf { int unused; };
struct Call {
    uint64_t at, members, good;
    bool operator<(const Call &o) const { return at < o.at; }
};
static const unsigned char *g_file = nullptr;
static std::mutex g_calls_mutex;
static std::vector<Call> g_calls;
extern "C" int flx_bgzf_inflate(flx_bgzf *, const void *in, const uint64_t *in_off, const uint64_t *out_off, uint64_t n, void *out,
                                uint64_t *first_bad) {
    static thread_local bgzf_inf::Shared S;
    *first_bad = n;
    for (uint64_t k = 0; k < n; ++k) {
        const uint32_t st = bgzf_inf::inflate_member_host(S, (const uint8_t *)in + in_off[k], (uint32_t)(in_off[k + 1] - in_off[k]),
                                                         out_off[k + 1] - out_off[k], (uint8_t *)out + out_off[k]);
        if (st != 0) { *first_bad = k; break; }
    }
    std::lock_guard<std::mutex> g(g_calls_mutex);  // (which runs the inflater gets, and how many members per call)
    g_calls.push_back({(uint64_t)((const unsigned char *)in - g_file), n, *first_bad});
    return FLX_OK;
}

static uint64_t fnv(uint64_t h, const char *p, size_t n) {
    for (size_t i = 0; i < n; ++i) h = (h ^ (unsigned char)p[i]) * 1099511628211ull;
    return h;
}

int main(int argc, char **argv) {
    if (argc < 5) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<unsigned char> file;
    char block[65536];
    for (size_t m; (m = fread(block, 1, sizeof block, f)) > 0;) file.insert(file.end(), block, block + m);
    fclose(f);
    const unsigned threads = (unsigned)atoi(argv[2]);
    const size_t want = (size_t)atoll(argv[3]);
    const uint64_t span = (uint64_t)atoll(argv[4]);
    g_file = file.data();
    flx_bgzf dev;
    ParallelInflate z;
    if (argc > 5 && strcmp(argv[5], "device") == 0) z.set_device(&dev);
    if (!z.open(file.data(), file.size(), file.size() >= 2 && file[0] == 0x1f && file[1] == 0x8b, threads)) { printf("open failed\n"); return 0; }
    std::vector<char> buf(32768 + want);
    std::vector<GzPoint> points;
    uint64_t digest = 1469598103934665603ull, total = 0, reads = 0, short_reads = 0;
    while (!z.eof() && !z.error()) {
        const size_t m = z.read(buf.data() + 32768, want, &points, span);
        digest = fnv(digest, buf.data() + 32768, m);
        total += m;
        ++reads;
        short_reads += m < want;
        if (m == 0 && !z.eof() && !z.error()) { printf("stalled\n"); return 1; }
        // (the reader's contract: the 32 KiB in front of the next write position are the stream's last)
        const size_t keep = std::min<size_t>(32768, m);
        memmove(buf.data() + 32768 - keep, buf.data() + 32768 + m - keep, keep);
    }
    printf("bytes %llu digest %016llx reads %llu short %llu\n", (unsigned long long)total, (unsigned long long)digest,
           (unsigned long long)reads, (unsigned long long)short_reads);
    for (const GzPoint &p : points)
        printf("point in %llu out %llu bits %d raw %d check %d member_base %llu crc %08lx window %zu %016llx\n", (unsigned long long)p.in,
               (unsigned long long)p.out, p.bits, (int)p.raw, (int)p.check, (unsigned long long)p.member_base, p.crc, p.window.size(),
               (unsigned long long)fnv(1469598103934665603ull, p.window.data(), p.window.size()));
    printf("eof %d error %d deliverable %llu total_out %llu\n", (int)z.eof(), (int)z.error(),
           (unsigned long long)(z.error() ? z.deliverable() : 0), (unsigned long long)z.total_out());
    printf("parallel %llu zlib_tail %llu rounds %u dropped %u device_members %llu\n", (unsigned long long)z.parallel_bytes(),
           (unsigned long long)z.zlib_tail_bytes(), z.rounds(), z.dropped_chunks(), (unsigned long long)z.device_members());
    std::sort(g_calls.begin(), g_calls.end());  // (the calls of a round come from several threads)
    for (const Call &c : g_calls)
        printf("device call at %llu members %llu good %llu\n", (unsigned long long)c.at, (unsigned long long)c.members, (unsigned long long)c.good);
    return 0;
}
