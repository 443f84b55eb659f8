// screen_host.cpp — the host core of --exclude (csrc/screen.h) as a stand-alone program, for tests/test_screen_host.py:
//   screen_host threshold P           prints t, or "invalid"
//   screen_host split IN OUT          IN: u64 n, then per sequence u64 length + its bytes; OUT: u64 pieces, then per piece u64 sequence,
//                                     u64 start inside the sequence, u64 length.  Every sequence sits in a heap block of exactly its
//                                     size (the sequences are handed over as one packed buffer WITHOUT a byte behind the last), so a
//                                     sanitized build sees any byte read outside them.
//   screen_host decide HITS WINDOWS T prints 1 or 0
//   screen_host bytes OUT             OUT: 256 bytes, 0xFF for a byte outside ACGTacgt, else its code
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "screen.h"

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
    if (argc == 3 && !strcmp(argv[1], "threshold")) {
        uint64_t t = 0;
        if (screen::threshold(atof(argv[2]), &t)) printf("%llu\n", (unsigned long long)t);
        else printf("invalid\n");
        return 0;
    }
    if (argc == 5 && !strcmp(argv[1], "decide")) {
        printf("%d\n", screen::excluded((uint32_t)strtoull(argv[2], nullptr, 10), (uint32_t)strtoull(argv[3], nullptr, 10), strtoull(argv[4], nullptr, 10)) ? 1 : 0);
        return 0;
    }
    if (argc == 3 && !strcmp(argv[1], "bytes")) {
        uint8_t out[256];
        for (int c = 0; c < 256; ++c) out[c] = screen::is_acgt((uint8_t)c) ? (uint8_t)screen::code_of((uint8_t)c) : 0xFF;
        FILE *f = fopen(argv[2], "wb");
        if (!f || fwrite(out, 1, 256, f) != 256) return 2;
        fclose(f);
        return 0;
    }
    if (argc == 4 && !strcmp(argv[1], "split")) {
        const std::vector<uint8_t> in = slurp(argv[2]);
        size_t at = 0;
        auto u64 = [&]() {
            uint64_t v;
            memcpy(&v, in.data() + at, 8);
            at += 8;
            return v;
        };
        const uint64_t n = u64();
        std::vector<uint64_t> offsets(n);
        std::vector<int64_t> lengths(n);
        uint64_t total = 0;
        size_t scan = at;
        for (uint64_t i = 0; i < n; ++i) {
            uint64_t len;
            memcpy(&len, in.data() + scan, 8);
            scan += 8 + len;
            offsets[i] = total;
            lengths[i] = (int64_t)len;
            total += len;
        }
        uint8_t *bases = (uint8_t *)malloc(total ? total : 1);  // exactly the sequences' bytes
        for (uint64_t i = 0; i < n; ++i) {
            const uint64_t len = u64();
            if (len) memcpy(bases + offsets[i], in.data() + at, len);
            at += len;
        }
        std::vector<uint64_t> po;
        std::vector<int64_t> pl;
        screen::split_acgt(total ? bases : nullptr, offsets.data(), lengths.data(), n, &po, &pl);
        FILE *f = fopen(argv[3], "wb");
        if (!f) return 2;
        const uint64_t np = po.size();
        fwrite(&np, 8, 1, f);
        for (uint64_t k = 0; k < np; ++k) {
            uint64_t s = 0;  // the sequence that holds the piece (an empty sequence holds none)
            while (!(po[k] >= offsets[s] && po[k] + (uint64_t)pl[k] <= offsets[s] + (uint64_t)lengths[s] && lengths[s] > 0)) ++s;
            const uint64_t rec[3] = {s, po[k] - offsets[s], (uint64_t)pl[k]};
            fwrite(rec, 8, 3, f);
        }
        fclose(f);
        free(bases);
        return 0;
    }
    return 2;
}
