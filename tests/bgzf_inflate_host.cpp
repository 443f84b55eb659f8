// bgzf_inflate_host.cpp — the member decoder of filtlong_amd/csrc/bgzf_inflate_member.h run on the host: every phase walks its
// lanes in order, the barriers fall between the phases (inflate_member_host).  bgzf_inflate_host CORPUS OUT reads
//   u32 n, then n times: u32 msize, u32 want_out, msize bytes (the member)
// and writes, per member, u32 status, u32 want_out, want_out bytes (0xAB where the decoder wrote nothing).  Every member is
// copied to a heap block of exactly its size at each of the alignments 0..3, so that a sanitizer build sees any read outside
// the member; the outputs of the four copies must agree.  Compiled by tests/test_bgzf_inflate_host.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
struct uint4 { unsigned x, y, z, w; };  // (bgzf_member.h, which the decoder takes its CRC arithmetic from, loads with it)
#include "bgzf_inflate_member.h"  // -I filtlong_amd/csrc
using namespace bgzf_inf;

static uint32_t get32(FILE *f) {
    uint8_t b[4];
    if (fread(b, 1, 4, f) != 4) { fprintf(stderr, "short corpus\n"); exit(2); }
    return rd32(b);
}
static void put32(FILE *f, uint32_t v) {
    const uint8_t b[4] = {(uint8_t)v, (uint8_t)(v >> 8), (uint8_t)(v >> 16), (uint8_t)(v >> 24)};
    fwrite(b, 1, 4, f);
}

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb"), *g = fopen(argv[2], "wb");
    if (!f || !g) return 2;
    const uint32_t n = get32(f);
    static Shared S;
    for (uint32_t k = 0; k < n; ++k) {
        const uint32_t msize = get32(f), want = get32(f);
        std::vector<uint8_t> mem(msize);
        if (msize && fread(mem.data(), 1, msize, f) != msize) return 2;
        std::vector<uint8_t> first;
        uint32_t first_st = 0;
        for (int a = 0; a < 4; ++a) {
            // operator new[] gives 16-byte alignment: the member starts at alignment a mod 4 and ends where the block ends
            const size_t pad = (size_t)a;
            uint8_t *blk = new uint8_t[pad + msize];
            uint8_t *m = blk + pad;
            if (msize) memcpy(m, mem.data(), msize);
            uint8_t *dst = new uint8_t[want ? want : 1];
            memset(dst, 0xAB, want ? want : 1);
            const uint32_t st = inflate_member_host(S, m, msize, want, dst);
            std::vector<uint8_t> got(dst, dst + want);
            delete[] dst;
            delete[] blk;
            if (a == 0) { first = got; first_st = st; }
            else if (st != first_st || got != first) { fprintf(stderr, "member %u: alignment %d differs\n", k, a); return 3; }
        }
        put32(g, first_st);
        put32(g, want);
        if (want) fwrite(first.data(), 1, want, g);
    }
    fclose(f);
    return fclose(g) == 0 ? 0 : 2;
}
