// complexity_host.cpp — the host core of --max_low_complexity (csrc/complexity.h) as a stand-alone program, for
// tests/test_complexity_host.py:
//   complexity_host walk IN OUT   IN: u32 T, u32 span, u64 n, then per read u64 length + its bytes; OUT per read: i32 S of its first
//                                 window from scratch (-1: a byte outside ACGTacgt, -2: no window), u32 windows, u32 bad windows of
//                                 the whole-read walk, of the walk in pieces of 64, of the walk in pieces of `span` and of the
//                                 walk in the kernel's spans and lane runs, u32 bad(S, T) of the first window.  Every read sits in
//                                 a heap block of exactly its size, so a sanitized build sees any byte read outside it.
//   complexity_host consts        prints window, warm-up, lane run and span
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "complexity.h"

static std::vector<uint8_t> slurp(const char *path) {
    FILE *f = fopen(path, "rb");
    if (!f) exit(2);
    std::vector<uint8_t> v;
    uint8_t buf[65536];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + n);
    fclose(f);
    return v;
}

int main(int argc, char **argv) {
    if (argc == 2 && !strcmp(argv[1], "consts")) {
        printf("%d %d %d %d\n", complexity::kWindow, complexity::kWarmup, complexity::kLaneRun, complexity::kSpan);
        return 0;
    }
    if (argc == 4 && !strcmp(argv[1], "walk")) {
        const std::vector<uint8_t> in = slurp(argv[2]);
        size_t at = 0;
        uint32_t T, span;
        uint64_t n;
        memcpy(&T, in.data(), 4);
        memcpy(&span, in.data() + 4, 4);
        memcpy(&n, in.data() + 8, 8);
        at = 16;
        FILE *f = fopen(argv[3], "wb");
        if (!f) return 2;
        for (uint64_t i = 0; i < n; ++i) {
            uint64_t len;
            memcpy(&len, in.data() + at, 8);
            at += 8;
            uint8_t *s = (uint8_t *)malloc(len ? len : 1);  // exactly the read's bytes (a read of no base: a block nobody reads)
            if (len) memcpy(s, in.data() + at, len);
            at += len;
            const uint8_t *read = len ? s : nullptr;
            const int32_t S0 = len >= (uint64_t)complexity::kWindow ? complexity::score_of_window(read) : -2;
            const uint32_t rec[6] = {complexity::windows_of((int64_t)len), complexity::bad_windows(read, (int64_t)len, T),
                                     complexity::bad_windows_pieces(read, (int64_t)len, T, complexity::kWindow),
                                     complexity::bad_windows_pieces(read, (int64_t)len, T, (int64_t)span),
                                     complexity::bad_windows_lanes(read, (int64_t)len, T),
                                     (S0 >= 0 && complexity::bad((uint32_t)S0, T)) ? 1u : 0u};
            fwrite(&S0, 4, 1, f);
            fwrite(rec, 4, 6, f);
            free(s);
        }
        fclose(f);
        return at == in.size() ? 0 : 2;
    }
    return 2;
}
