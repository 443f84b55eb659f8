// pinflate_device_host.cpp — ParallelInflate (filtlong_amd/cli/pinflate.h) with a device inflater, without a device: flx_bgzf_inflate
// is defined here over the host walk of bgzf_inflate_member.h, which gives the kernel's status words and bytes.  The program reads
// FILE through ParallelInflate twice, with a null object and with this one, and compares everything a caller can see: the bytes,
// eof(), error() and deliverable().  It prints "same BYTES device DEVICE_MEMBERS" or says what differs (exit 1).
// Compiled by tests/test_pinflate_device_host.py; FLX_CLI_PINFLATE_MIN / _CHUNK make the parallel reader take a small file.
#include <cstdio>
#include <string>
#include <vector>
struct uint4 { unsigned x, y, z, w; };
#include "bgzf_inflate_member.h"  // -I filtlong_amd/csrc
#include "pinflate.h"             // -I filtlong_amd/cli

struct flx_bgzf { int unused; };
extern "C" int flx_bgzf_inflate(flx_bgzf *, const void *in, const uint64_t *in_off, const uint64_t *out_off, uint64_t n, void *out,
                                uint64_t *first_bad) {
    static thread_local bgzf_inf::Shared S;
    *first_bad = n;
    for (uint64_t k = 0; k < n; ++k) {
        const uint32_t st = bgzf_inf::inflate_member_host(S, (const uint8_t *)in + in_off[k], (uint32_t)(in_off[k + 1] - in_off[k]),
                                                         out_off[k + 1] - out_off[k], (uint8_t *)out + out_off[k]);
        if (st != 0) { *first_bad = k; break; }
    }
    return FLX_OK;
}

struct Seen {
    std::string bytes;
    bool eof = false, error = false;
    uint64_t deliverable = 0, device_members = 0;
};
static bool read_all(const std::vector<unsigned char> &file, flx_bgzf *dev, Seen &s) {
    ParallelInflate z;
    z.set_device(dev);
    if (!z.open(file.data(), file.size(), true, 4)) { s.error = true; return true; }
    std::vector<char> buf((size_t)70000 + 32768);
    while (!z.eof() && !z.error()) {
        const size_t m = z.read(buf.data() + 32768, 70000);
        s.bytes.append(buf.data() + 32768, m);
        if (m == 0 && !z.eof() && !z.error()) return false;
    }
    s.eof = z.eof();
    s.error = z.error();
    s.deliverable = z.error() ? z.deliverable() : 0;
    s.device_members = z.device_members();
    return true;
}

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<unsigned char> file;
    int c;
    while ((c = fgetc(f)) != EOF) file.push_back((unsigned char)c);
    fclose(f);
    flx_bgzf dev;
    Seen host, device;
    if (!read_all(file, nullptr, host) || !read_all(file, &dev, device)) { printf("stalled\n"); return 1; }
    if (host.bytes != device.bytes) { printf("bytes differ: %zu host, %zu device\n", host.bytes.size(), device.bytes.size()); return 1; }
    if (host.eof != device.eof || host.error != device.error || host.deliverable != device.deliverable) {
        printf("end differs: eof %d/%d error %d/%d deliverable %llu/%llu\n", host.eof, device.eof, host.error, device.error,
               (unsigned long long)host.deliverable, (unsigned long long)device.deliverable);
        return 1;
    }
    if (host.device_members != 0) { printf("the null object counted device members\n"); return 1; }
    printf("same %zu error %d device %llu\n", host.bytes.size(), (int)host.error, (unsigned long long)device.device_members);
    return 0;
}
