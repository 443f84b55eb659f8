// bam_encode_host.cpp — the record core of filtlong_amd/csrc/bam_encode.h walked on the host.  bam_encode_host CORPUS OUT reads
//   u32 n, then n times: u32 records, records + 1 offsets (u64), u32 size, size bytes of record text
// and writes, per case: u64 first bad record, u64 BAM length, the BAM records, records + 1 BAM offsets (u64), then the round trip:
// u64 text length and the text bam_record.h's host walk gives for the encoded records.  Every text is copied to a heap block of
// exactly its size and the records go to a block of exactly their length, so that a sanitizer build sees any access outside
// either.  Compiled by tests/test_bam_encode_host.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "bam_encode.h"  // -I filtlong_amd/csrc
#include "bam_record.h"

static uint32_t get32(FILE *f) {
    uint8_t b[4];
    if (fread(b, 1, 4, f) != 4) { fprintf(stderr, "short corpus\n"); exit(2); }
    return bam::rd32(b);
}
static uint64_t get64(FILE *f) {
    const uint64_t lo = get32(f);
    return lo | (uint64_t)get32(f) << 32;
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
        const uint32_t records = get32(f);
        std::vector<uint64_t> off(records + 1), out_off(records + 1);
        for (uint64_t &o : off) o = get64(f);
        const uint32_t size = get32(f);
        uint8_t *text = new uint8_t[size];
        if (size && fread(text, 1, size, f) != size) return 2;
        uint64_t first_bad = 0;
        const uint64_t len = bamenc::sizes_host(text, size, off.data(), records, out_off.data(), &first_bad);
        uint8_t *rec = new uint8_t[len];
        bamenc::emit_records_host(text, size, off.data(), records, rec);
        put64(g, first_bad);
        put64(g, len);
        if (len) fwrite(rec, 1, len, g);
        for (uint64_t o : out_off) put64(g, o);
        // the way back: records of invalid shape took no bytes, so their ranges are empty and give no text
        uint64_t back_len = 0;
        for (uint32_t r = 0; r < records; ++r)
            if (out_off[r + 1] > out_off[r]) back_len += bam::text_bytes_host(rec, out_off.data(), r, r + 1, nullptr);
        uint8_t *back = new uint8_t[back_len];
        uint8_t *at = back;
        for (uint32_t r = 0; r < records; ++r)
            if (out_off[r + 1] > out_off[r]) {
                bam::emit_records_host(rec, out_off.data(), r, r + 1, at);
                at += bam::text_bytes_host(rec, out_off.data(), r, r + 1, nullptr);
            }
        put64(g, back_len);
        if (back_len) fwrite(back, 1, back_len, g);
        delete[] back;
        delete[] rec;
        delete[] text;
    }
    fclose(f);
    return fclose(g) == 0 ? 0 : 2;
}
