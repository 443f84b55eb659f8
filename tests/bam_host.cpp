// bam_host.cpp — the record core of filtlong_amd/csrc/bam_record.h walked on the host.  bam_host CORPUS OUT reads
//   u32 n, then n times: u32 size, size bytes (an inflated BAM file, good or damaged)
// and writes, per file: u32 end state, u64 records, u64 skipped records, u64 text length, the text, then records + 1 text offsets
// (u64).  Every file is copied to a heap block of exactly its size and the text goes to a block of exactly its length, so that a
// sanitizer build sees any access outside either.  The records in front of a truncation or a bad record are still turned into text.
// Compiled by tests/test_bam_host.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "bam_record.h"  // -I filtlong_amd/csrc

static uint32_t get32(FILE *f) {
    uint8_t b[4];
    if (fread(b, 1, 4, f) != 4) { fprintf(stderr, "short corpus\n"); exit(2); }
    return bam::rd32(b);
}
static void put64(FILE *f, uint64_t v) {
    uint8_t b[8];
    for (int i = 0; i < 8; ++i) b[i] = (uint8_t)(v >> (8 * i));
    fwrite(b, 1, 8, f);
}

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb"), *g = fopen(argv[2], "wb");
    if (!f || !g) return 2;
    const uint32_t n = get32(f);
    for (uint32_t k = 0; k < n; ++k) {
        const uint32_t size = get32(f);
        uint8_t *file = new uint8_t[size];
        if (size && fread(file, 1, size, f) != size) return 2;
        uint64_t records = 0, again = 0, skipped = 0;
        const int end = bam::index_host(file, size, UINT64_MAX, nullptr, &records);
        std::vector<uint64_t> off(records + 1);
        (void)bam::index_host(file, size, records, off.data(), &again);
        if (again != records) { fprintf(stderr, "file %u: the second walk differs\n", k); return 3; }
        const uint64_t len = bam::text_bytes_host(file, off.data(), 0, records, &skipped);
        uint8_t *text = new uint8_t[len];
        bam::emit_records_host(file, off.data(), 0, records, text);
        const uint8_t e[4] = {(uint8_t)end, 0, 0, 0};
        fwrite(e, 1, 4, g);
        put64(g, records);
        put64(g, skipped);
        put64(g, len);
        if (len) fwrite(text, 1, len, g);
        uint64_t at = 0;
        put64(g, 0);
        for (uint64_t r = 0; r < records; ++r) {
            at += bam::text_bytes_host(file, off.data(), r, r + 1, nullptr);
            put64(g, at);
        }
        delete[] text;
        delete[] file;
    }
    fclose(f);
    return fclose(g) == 0 ? 0 : 2;
}
