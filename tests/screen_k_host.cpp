// screen_k_host.cpp — the host core of --exclude_k (csrc/screen_hash.h) as a stand-alone program, for tests/test_screen_k_host.py:
//   screen_k_host keys K IN OUT      IN: the bytes of one sequence; OUT: per window u8 valid, u64 forward code, u64 reverse-complement
//                                    code, u64 canonical key (zeros for a window that is not valid).  The sequence sits in a heap
//                                    block of exactly its size, so a sanitized build sees any byte read outside it.
//   screen_k_host windows L K        prints windows_of(L, K)
//   screen_k_host table CAP IN OUT   IN: u64 n, then n times u8 op ('i' insert, 'f' find) + u64 key; the table has CAP slots and
//                                    starts empty.  OUT: per op an i64 (insert: 1 / 0 / -1, find: the slot, or CAP), then the CAP
//                                    slots of the table.
//   screen_k_host slot KEY CAP       prints slot_of(KEY, CAP)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "screen_hash.h"

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
    if (argc == 4 && !strcmp(argv[1], "windows")) {
        printf("%u\n", screenk::windows_of(atoll(argv[2]), atoi(argv[3])));
        return 0;
    }
    if (argc == 4 && !strcmp(argv[1], "slot")) {
        printf("%llu\n", (unsigned long long)screenk::slot_of(strtoull(argv[2], nullptr, 10), strtoull(argv[3], nullptr, 10)));
        return 0;
    }
    if (argc == 5 && !strcmp(argv[1], "keys")) {
        const int k = atoi(argv[2]);
        const std::vector<uint8_t> in = slurp(argv[3]);
        uint8_t *seq = (uint8_t *)malloc(in.size() ? in.size() : 1);  // exactly the sequence's bytes
        if (!in.empty()) memcpy(seq, in.data(), in.size());
        FILE *f = fopen(argv[4], "wb");
        if (!f) return 2;
        const uint32_t n = screenk::windows_of((int64_t)in.size(), k);
        for (uint32_t i = 0; i < n; ++i) {
            uint8_t valid = screenk::window_valid(seq + i, k) ? 1 : 0;
            uint64_t rec[3] = {0, 0, 0};
            if (valid) {
                rec[0] = screenk::forward_code(seq + i, k);
                rec[1] = screenk::revcomp_code(rec[0], k);
                rec[2] = screenk::canonical(rec[0], k);
            }
            fwrite(&valid, 1, 1, f);
            fwrite(rec, 8, 3, f);
        }
        fclose(f);
        free(seq);
        return 0;
    }
    if (argc == 5 && !strcmp(argv[1], "table")) {
        const uint64_t cap = strtoull(argv[2], nullptr, 10);
        const std::vector<uint8_t> in = slurp(argv[3]);
        uint64_t n;
        memcpy(&n, in.data(), 8);
        uint64_t *table = (uint64_t *)malloc(cap * 8);  // exactly the table's slots
        for (uint64_t s = 0; s < cap; ++s) table[s] = screenk::kEmpty;
        FILE *f = fopen(argv[4], "wb");
        if (!f) return 2;
        for (uint64_t i = 0; i < n; ++i) {
            const uint8_t op = in[8 + 9 * i];
            uint64_t key;
            memcpy(&key, in.data() + 8 + 9 * i + 1, 8);
            const int64_t r = op == 'i' ? (int64_t)screenk::insert(table, cap, key) : (int64_t)screenk::find(table, cap, key);
            fwrite(&r, 8, 1, f);
        }
        fwrite(table, 8, cap, f);
        fclose(f);
        free(table);
        return 0;
    }
    return 2;
}
