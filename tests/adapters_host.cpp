// adapters_host.cpp — the host walk of --trim_adapters (csrc/adapters.h) as a stand-alone program, for tests/test_adapters_host.py:
//   adapters_host run IN OUT   IN: i32 E, i32 W, u64 sequences, per sequence u64 length + its bytes, u64 reads, per read u64 length + its
//                              bytes.  OUT: i64 what adapters::build returned; when that is 0: u64 patterns, per pattern u32 m, u32 k, its
//                              m bases as the head masks spell them and its m bases as the tail masks spell them; then per read u32 head
//                              key, u32 tail key, i32 children, i32 first, i32 last.
//                              Every read sits in a heap block of exactly its size, and so do the sequences (one packed buffer WITHOUT a
//                              byte behind the last), so a sanitized build sees any byte read outside them.
//   adapters_host bytes OUT    OUT: 256 bytes, the code of every byte value (4 for a byte outside ACGTacgt)
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

// the bases the four masks spell (bit i set in exactly one of them, for i < m)
static void spell(const uint64_t peq[4], uint32_t m, FILE *f) {
    for (uint32_t i = 0; i < m; ++i) {
        char c = '?';
        int seen = 0;
        for (int b = 0; b < 4; ++b)
            if ((peq[b] >> i) & 1u) {
                c = "ACGT"[b];
                ++seen;
            }
        if (seen != 1) c = '!';
        fputc(c, f);
    }
    for (int b = 0; b < 4; ++b)
        if (m < 64 && (peq[b] >> m)) exit(3);  // nothing above the pattern
}

int main(int argc, char **argv) {
    if (argc == 3 && !strcmp(argv[1], "bytes")) {
        uint8_t out[256];
        for (int c = 0; c < 256; ++c) out[c] = (uint8_t)adapters::code_of((uint8_t)c);
        FILE *f = fopen(argv[2], "wb");
        if (!f || fwrite(out, 1, 256, f) != 256) return 2;
        fclose(f);
        return 0;
    }
    if (argc == 4 && !strcmp(argv[1], "run")) {
        const std::vector<uint8_t> in = slurp(argv[2]);
        size_t at = 0;
        auto u64 = [&]() {
            uint64_t v;
            memcpy(&v, in.data() + at, 8);
            at += 8;
            return v;
        };
        int32_t ew[2];
        memcpy(ew, in.data(), 8);
        at = 8;
        const uint64_t n_seqs = u64();
        std::vector<uint64_t> offsets(n_seqs);
        std::vector<int64_t> lengths(n_seqs);
        uint64_t total = 0;
        size_t scan = at;
        for (uint64_t i = 0; i < n_seqs; ++i) {
            uint64_t len;
            memcpy(&len, in.data() + scan, 8);
            scan += 8 + len;
            offsets[i] = total;
            lengths[i] = (int64_t)len;
            total += len;
        }
        uint8_t *bases = (uint8_t *)malloc(total ? total : 1);  // exactly the sequences' bytes
        for (uint64_t i = 0; i < n_seqs; ++i) {
            const uint64_t len = u64();
            if (len) memcpy(bases + offsets[i], in.data() + at, len);
            at += len;
        }
        std::vector<adapters::Pattern> pats;
        const int64_t rc = adapters::build(bases, offsets.data(), lengths.data(), n_seqs, ew[0], ew[1], &pats);
        free(bases);
        FILE *f = fopen(argv[3], "wb");
        if (!f) return 2;
        fwrite(&rc, 8, 1, f);
        if (rc == 0) {
            const uint64_t np = pats.size();
            fwrite(&np, 8, 1, f);
            for (const adapters::Pattern &p : pats) {
                fwrite(&p.m, 4, 1, f);
                fwrite(&p.k, 4, 1, f);
                spell(p.peq_head, p.m, f);
                spell(p.peq_tail, p.m, f);
            }
            const uint64_t n_reads = u64();
            for (uint64_t r = 0; r < n_reads; ++r) {
                const uint64_t len = u64();
                uint8_t *read = (uint8_t *)malloc(len ? len : 1);  // exactly the read's bytes
                if (len) memcpy(read, in.data() + at, len);
                at += len;
                const uint32_t keys[2] = {adapters::end_key(len ? read : nullptr, (int64_t)len, 0, ew[1], pats.data(), (uint32_t)np),
                                          adapters::end_key(len ? read : nullptr, (int64_t)len, 1, ew[1], pats.data(), (uint32_t)np)};
                int32_t c[3];
                c[0] = adapters::child_of(keys[0], keys[1], (int64_t)len, &c[1], &c[2]);
                fwrite(keys, 4, 2, f);
                fwrite(c, 4, 3, f);
                free(read);
            }
        }
        fclose(f);
        return 0;
    }
    return 2;
}
