// adapters_split_host.cpp — the host walk of --split_adapters (csrc/adapters.h) as a stand-alone program, for
// tests/test_adapters_split_host.py:
//   adapters_split_host IN OUT   IN: i32 E, i32 W, i32 E2, i32 pad, u64 sequences, per sequence u64 length + its bytes, u64 reads, per read
//                                u64 length + its bytes.  OUT: i64 what adapters::build returned; when that is 0, per read: u32 head key,
//                                u32 tail key, i32 children, i32 first, i32 last, the children as i32 pairs, then three times L bytes
//                                (0 or 1 per base): the marks of the whole-read walk, of the piece-wise walk with S = 64 and with S = 1024.
//                                Every read sits in a heap block of exactly its size and so do its marks, so a sanitized build sees any
//                                byte touched outside them.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "adapters.h"

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
    if (argc != 3) return 2;
    const std::vector<uint8_t> in = slurp(argv[1]);
    size_t at = 0;
    auto u64 = [&]() {
        uint64_t v;
        memcpy(&v, in.data() + at, 8);
        at += 8;
        return v;
    };
    int32_t head[4];
    memcpy(head, in.data(), 16);
    at = 16;
    const int errors = head[0], window = head[1], split_errors = head[2];
    const uint64_t n_seqs = u64();
    std::vector<uint64_t> offsets(n_seqs);
    std::vector<int64_t> lengths(n_seqs);
    std::vector<uint8_t> bases;
    for (uint64_t i = 0; i < n_seqs; ++i) {
        const uint64_t len = u64();
        offsets[i] = bases.size();
        lengths[i] = (int64_t)len;
        bases.insert(bases.end(), in.data() + at, in.data() + at + len);
        at += len;
    }
    std::vector<adapters::Pattern> pats;
    const int64_t rc = adapters::build(bases.data(), offsets.data(), lengths.data(), n_seqs, errors, window, &pats);
    FILE *f = fopen(argv[2], "wb");
    if (!f) return 2;
    fwrite(&rc, 8, 1, f);
    if (rc == 0) {
        const uint32_t np = (uint32_t)pats.size();
        const uint64_t n_reads = u64();
        for (uint64_t r = 0; r < n_reads; ++r) {
            const uint64_t len = u64();
            uint8_t *read = (uint8_t *)malloc(len ? len : 1);  // exactly the read's bytes
            if (len) memcpy(read, in.data() + at, len);
            at += len;
            const uint8_t *rp = len ? read : nullptr;
            uint8_t *marked[3];
            for (int k = 0; k < 3; ++k) marked[k] = (uint8_t *)calloc(len ? len : 1, 1);
            adapters::middle_marks(rp, (int64_t)len, pats.data(), np, (uint32_t)split_errors, marked[0]);
            adapters::middle_marks_pieces(rp, (int64_t)len, 64, pats.data(), np, (uint32_t)split_errors, marked[1]);
            adapters::middle_marks_pieces(rp, (int64_t)len, 1024, pats.data(), np, (uint32_t)split_errors, marked[2]);
            const uint32_t keys[2] = {adapters::end_key(rp, (int64_t)len, 0, window, pats.data(), np),
                                      adapters::end_key(rp, (int64_t)len, 1, window, pats.data(), np)};
            std::vector<int32_t> ranges;
            int32_t c[3];
            c[0] = (int32_t)adapters::split_children(keys[0], keys[1], (int64_t)len, marked[0], &ranges, &c[1], &c[2]);
            fwrite(keys, 4, 2, f);
            fwrite(c, 4, 3, f);
            if (!ranges.empty()) fwrite(ranges.data(), 4, ranges.size(), f);
            for (int k = 0; k < 3; ++k) {
                if (len) fwrite(marked[k], 1, len, f);
                free(marked[k]);
            }
            free(read);
        }
    }
    fclose(f);
    return 0;
}
