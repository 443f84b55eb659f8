// bgzf_host.cpp — the member encoder of filtlong_amd/csrc/bgzf_member.h run on the host: every phase walks its threads
// in order, the barriers fall between the phases.  bgzf_host IN OUT writes the BGZF stream (with the end-of-file block)
// that k_bgzf_members + k_bgzf_gather write for IN.  Compiled by tests/test_bgzf_format.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
struct uint4 { unsigned x, y, z, w; };
#include "bgzf_member.h"  // -I filtlong_amd/csrc
using namespace bgzf;
int main(int argc, char **argv) {
    FILE *f = fopen(argv[1], "rb"); std::vector<uint8_t> in; int c;
    while ((c = fgetc(f)) != EOF) in.push_back((uint8_t)c);
    fclose(f);
    uint64_t N = in.size();
    static Shared S;
    std::vector<uint32_t> mt(BG_MEMBER);
    std::vector<uint8_t> slot(BG_SLOT), out;
    for (uint64_t off = 0; off < N; off += BG_MEMBER) {
        uint32_t n = N - off < BG_MEMBER ? N - off : BG_MEMBER;
        const uint8_t *src = in.data() + off;
        std::fill(slot.begin(), slot.end(), 0xAB);
        for (int t = 0; t < BG_NT; ++t) ph_load(t, S, src, n, false);
        for (int t = 0; t < BG_NT; ++t) ph_crc(t, S, n);
        for (int t = 0; t < BG_NT; ++t) ph_crc_final(t, S, n);
        for (uint32_t base = 0; base < n; base += BG_NT) {
            for (int t = 0; t < BG_NT; ++t) ph_lookup(t, S, n, base, mt.data());
            for (int t = 0; t < BG_NT; ++t) ph_insert(t, S, n, base);
        }
        for (int t = 0; t < BG_NT; ++t) ph_hist(t, S, n, mt.data());
        for (int t = 0; t < BG_NT; ++t) ph_rank(t, S);
        for (int t = 0; t < BG_NT; ++t) ph_codes(t, S);
        for (int t = 0; t < BG_NT; ++t) ph_header(t, S, n);
        for (int t = 0; t < BG_NT; ++t) ph_count(t, S, n, mt.data());
        for (int t = 0; t < BG_NT; ++t) ph_scan(t, S);
        for (int t = 0; t < BG_NT; ++t) ph_zero(t, S, slot.data());
        for (int t = 0; t < BG_NT; ++t) ph_pack(t, S, n, mt.data(), slot.data());
        uint32_t sz = 0;
        for (int t = 0; t < BG_NT; ++t) ph_frame(t, S, n, slot.data(), &sz);
        for (uint32_t j = 0; j < sz; ++j) out.push_back(j < 18 ? slot[j] : slot[BG_DEFL_OFF + j - 18]);
    }
    const uint8_t eof[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    out.insert(out.end(), eof, eof + 28);
    f = fopen(argv[2], "wb"); fwrite(out.data(), 1, out.size(), f); fclose(f);
    return 0;
}
