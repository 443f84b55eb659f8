// adapters_overhang_host.cpp — the host walks of --adapter_overhang (csrc/adapters.h) as a stand-alone program, for
// tests/test_adapters_overhang_host.py:
//   adapters_overhang_host IN OUT   IN: i32 E, i32 W, i32 O, i32 0, u64 sequences, per sequence u64 length + its bytes, u64 reads, per
//                                   read u64 length + its bytes.  OUT: i64 what adapters::build returned, i64 whether
//                                   adapters::set_overhang took O; when both are fine: u64 patterns, per pattern u32 m, k, o, k_o; then
//                                   per read u32 head key, u32 tail key.
//                                   Every read sits in a heap block of exactly its size, so a sanitized build sees any byte read
//                                   outside it.
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
    int32_t ewo[4];
    memcpy(ewo, in.data(), 16);
    at = 16;
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
    const int64_t rc = adapters::build(bases.data(), offsets.data(), lengths.data(), n_seqs, ewo[0], ewo[1], &pats);
    const int64_t took = rc == 0 && adapters::set_overhang(&pats, ewo[0], ewo[2]) ? 1 : 0;
    FILE *f = fopen(argv[2], "wb");
    if (!f) return 2;
    fwrite(&rc, 8, 1, f);
    fwrite(&took, 8, 1, f);
    if (rc == 0 && took) {
        const uint64_t np = pats.size();
        fwrite(&np, 8, 1, f);
        for (const adapters::Pattern &p : pats) {
            const uint32_t v[4] = {p.m, p.k, p.o, p.k_o};
            fwrite(v, 4, 4, f);
        }
        const uint64_t n_reads = u64();
        for (uint64_t r = 0; r < n_reads; ++r) {
            const uint64_t len = u64();
            uint8_t *read = (uint8_t *)malloc(len ? len : 1);  // exactly the read's bytes
            if (len) memcpy(read, in.data() + at, len);
            at += len;
            const uint32_t keys[2] = {adapters::end_key(len ? read : nullptr, (int64_t)len, 0, ewo[1], pats.data(), (uint32_t)np),
                                      adapters::end_key(len ? read : nullptr, (int64_t)len, 1, ewo[1], pats.data(), (uint32_t)np)};
            fwrite(keys, 4, 2, f);
            free(read);
        }
    }
    fclose(f);
    return 0;
}
