// pinflate_alloc_host.cpp — an allocation that fails inside a round of the parallel gzip reader (filtlong_amd/cli/pinflate.h).
// Global operator new is replaced: while the reader is open, the k-th allocation of at least 64 KiB throws std::bad_alloc (the
// decoders' symbol buffers, the pieces' byte buffers and the BGZF runs' are all of that size; the program's own buffers are made
// before).  A clean run counts such allocations, K; then k = 1 .. K.  Every run must deliver exactly the bytes and the end state of
// InflateStream alone — the round that failed never happened, zlib reads on from where it began — and the process must live.
//   pinflate_alloc_host FILE THREADS [MIN_BYTES]     prints "ok K <K> failed <runs in which an allocation was made to fail> bytes <n>"
// MIN_BYTES (65536): with a smaller figure the buffers of later rounds count too, and a round fails that did not begin the member.
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <new>
#include <string>
#include <vector>
#include "pinflate.h"  // -I filtlong_amd/cli

struct flx_bgzf { int unused; };
extern "C" int flx_bgzf_inflate(flx_bgzf *, const void *, const uint64_t *, const uint64_t *, uint64_t, void *, uint64_t *) { return FLX_ERR_INVALID; }

static std::atomic<bool> g_armed{false};
static std::atomic<long> g_large{0}, g_fail_at{0}, g_failed{0};
static size_t g_min_bytes = 65536;

void *operator new(size_t n) {
    if (n >= g_min_bytes && g_armed) {
        const long k = ++g_large;
        if (k == g_fail_at) { ++g_failed; throw std::bad_alloc(); }
    }
    if (void *p = malloc(n ? n : 1)) return p;
    throw std::bad_alloc();
}
void *operator new[](size_t n) { return operator new(n); }
void operator delete(void *p) noexcept { free(p); }
void operator delete[](void *p) noexcept { free(p); }
void operator delete(void *p, size_t) noexcept { free(p); }
void operator delete[](void *p, size_t) noexcept { free(p); }

struct Seen {
    std::string bytes;
    bool eof = false, error = false;
    uint64_t deliverable = 0;
    bool operator==(const Seen &o) const { return bytes == o.bytes && eof == o.eof && error == o.error && deliverable == o.deliverable; }
};

template <class Reader>
static void drain(Reader &z, std::vector<char> &buf, Seen &s) {
    while (!z.eof() && !z.error()) {
        const size_t m = z.read(buf.data() + 32768, 70000);
        s.bytes.append(buf.data() + 32768, m);
        if (m == 0 && !z.eof() && !z.error()) break;
    }
    s.eof = z.eof();
    s.error = z.error();
    s.deliverable = z.error() ? z.deliverable() : 0;
}

int main(int argc, char **argv) {
    if (argc != 3 && argc != 4) return 2;
    if (argc == 4) g_min_bytes = (size_t)atoll(argv[3]);
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<unsigned char> file;
    int c;
    while ((c = fgetc(f)) != EOF) file.push_back((unsigned char)c);
    fclose(f);
    const unsigned threads = (unsigned)atoi(argv[2]);
    std::vector<char> buf((size_t)70000 + 32768);
    Seen want;
    {
        InflateStream z;
        if (!z.open(file.data(), file.size(), true)) { printf("FAILED: the serial reader does not open the file\n"); return 1; }
        drain(z, buf, want);
    }
    long K = 0, failed_runs = 0;
    for (long k = 0; k <= K; ++k) {  // k = 0: the clean run that counts
        Seen got;
        got.bytes.reserve(want.bytes.size() + 70000);
        unsigned rounds = 0;
        {
            ParallelInflate z;
            g_large = 0;
            g_failed = 0;
            g_fail_at = k;
            g_armed = true;
            const bool opened = z.open(file.data(), file.size(), true, threads);
            if (opened) drain(z, buf, got);
            g_armed = false;
            if (!opened) { printf("FAILED: k = %ld: open\n", k); return 1; }
            rounds = z.rounds();
        }
        if (k == 0) {
            K = g_large;
            if (rounds < 1) { printf("FAILED: the clean run went through no round\n"); return 1; }
        }
        failed_runs += g_failed;
        if (!(got == want)) {
            printf("FAILED: k = %ld of %ld: %zu bytes eof %d error %d deliverable %llu, InflateStream alone: %zu bytes eof %d error %d deliverable %llu\n",
                   k, K, got.bytes.size(), got.eof, got.error, (unsigned long long)got.deliverable, want.bytes.size(), want.eof, want.error,
                   (unsigned long long)want.deliverable);
            return 1;
        }
    }
    printf("ok K %ld failed %ld bytes %zu\n", K, failed_runs, want.bytes.size());
    return 0;
}
