// qsplit_host.cpp — the record core of --split_window_q (filtlong_amd/csrc/qsplit.h) walked on the host: a stand-alone program for
// tests/test_qsplit_host.py, built with -O2 and again with the address and undefined-behaviour sanitizers.
//   qsplit_host table OUT          the 256 entries of the error table, uint32 little-endian
//   qsplit_host threshold Q        prints t of --split_window_q Q, or "invalid"
//   qsplit_host walk IN OUT        IN: u32 count, then per case i64 W, u64 t, u64 L and L quality bytes.  Every quality string is
//                                  copied into a heap block of exactly its size before the walk (a read one byte outside is the
//                                  sanitizer's to find).  OUT per case: u64 children, i32 first, i32 last, u32 any_bad, the ranges.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "qsplit.h"

static bool read_file(const char *path, std::vector<uint8_t> &out) {
    FILE *f = fopen(path, "rb");
    if (!f) return false;
    uint8_t buf[1 << 16];
    size_t got;
    while ((got = fread(buf, 1, sizeof buf, f)) > 0) out.insert(out.end(), buf, buf + got);
    fclose(f);
    return true;
}

template <typename T>
static void put(std::vector<uint8_t> &out, T v) {
    const uint8_t *p = (const uint8_t *)&v;
    out.insert(out.end(), p, p + sizeof v);
}

int main(int argc, char **argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "table" && argc == 3) {
        FILE *f = fopen(argv[2], "wb");
        if (!f || fwrite(qsplit::kErrorTable, 4, 256, f) != 256) return 2;
        return fclose(f) == 0 ? 0 : 2;
    }
    if (mode == "threshold" && argc == 3) {
        uint64_t t = 0;
        if (qsplit::threshold(atof(argv[2]), &t)) printf("%llu\n", (unsigned long long)t);
        else printf("invalid\n");
        return 0;
    }
    if (mode != "walk" || argc != 4) {
        fprintf(stderr, "usage: qsplit_host table OUT | threshold Q | walk IN OUT\n");
        return 2;
    }
    std::vector<uint8_t> in, out;
    if (!read_file(argv[2], in) || in.size() < 4) return 2;
    uint32_t count;
    memcpy(&count, in.data(), 4);
    size_t at = 4;
    for (uint32_t c = 0; c < count; ++c) {
        if (at + 24 > in.size()) return 2;
        int64_t w;
        uint64_t t, l;
        memcpy(&w, &in[at], 8);
        memcpy(&t, &in[at + 8], 8);
        memcpy(&l, &in[at + 16], 8);
        at += 24;
        if (l > in.size() - at) return 2;
        uint8_t *qual = (uint8_t *)malloc(l ? l : 1);  // (exactly the read's size; one byte for an empty read, never touched)
        if (!qual) return 2;
        if (l) memcpy(qual, &in[at], l);
        at += l;
        qsplit::Children ch;
        qsplit::qsplit_children_host(l ? qual : nullptr, (int64_t)l, w, t, &ch);
        free(qual);
        put<uint64_t>(out, ch.ranges.size() / 2);
        put<int32_t>(out, ch.first);
        put<int32_t>(out, ch.last);
        put<uint32_t>(out, ch.any_bad ? 1u : 0u);
        for (int32_t v : ch.ranges) put<int32_t>(out, v);
    }
    FILE *f = fopen(argv[3], "wb");
    if (!f || (out.size() && fwrite(out.data(), 1, out.size(), f) != out.size())) return 2;
    return fclose(f) == 0 ? 0 : 2;
}
