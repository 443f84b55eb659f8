// endtrim_host.cpp — the host core of --trim_ends_q (csrc/endtrim.h) as a stand-alone program, for tests/test_endtrim_host.py:
//   endtrim_host walk IN OUT   IN: u64 t, u64 n, then per read u64 length + its bytes; OUT per read ten u32: h and c of the serial walk,
//                              then h and c of the walk in pieces of 1, 7, 64 and the span combined in order.  Every read sits in a
//                              heap block of exactly its size, so a sanitized build sees any byte read outside it.
//   endtrim_host consts        prints the span
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "endtrim.h"

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
        printf("%d\n", endtrim::kSpan);
        return 0;
    }
    if (argc == 4 && !strcmp(argv[1], "walk")) {
        const std::vector<uint8_t> in = slurp(argv[2]);
        uint64_t t, n;
        memcpy(&t, in.data(), 8);
        memcpy(&n, in.data() + 8, 8);
        size_t at = 16;
        FILE *f = fopen(argv[3], "wb");
        if (!f) return 2;
        const int64_t pieces[4] = {1, 7, 64, endtrim::kSpan};
        for (uint64_t i = 0; i < n; ++i) {
            uint64_t len;
            memcpy(&len, in.data() + at, 8);
            at += 8;
            uint8_t *s = (uint8_t *)malloc(len ? len : 1);  // exactly the read's bytes (a read of no base: a block nobody reads)
            if (len) memcpy(s, in.data() + at, len);
            at += len;
            const uint8_t *read = len ? s : nullptr;
            uint32_t rec[10];
            endtrim::cuts_host(read, (int64_t)len, t, &rec[0], &rec[1]);
            for (int k = 0; k < 4; ++k) endtrim::cuts_by_pieces(read, (int64_t)len, t, pieces[k], &rec[2 + 2 * k], &rec[3 + 2 * k]);
            fwrite(rec, 4, 10, f);
            free(s);
        }
        fclose(f);
        return at == in.size() ? 0 : 2;
    }
    return 2;
}
