// gzip_framing_host.cpp — filtlong_amd/csrc/gzip_framing.h on its own: what it says stands at byte 0 of each FILE.
//   gzip_framing_host FILE...            one line per file
//   gzip_framing_host --prefixes FILE    one line per prefix length 0 .. size of FILE
// Every buffer is a heap block of exactly the data's size, so that a read past the end is seen by the address sanitizer.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "gzip_framing.h"  // -I filtlong_amd/csrc

static void verdict(const std::vector<unsigned char> &bytes, size_t n) {
    unsigned char *d = (unsigned char *)malloc(n ? n : 1);
    if (n == 0) {  // (a block of no bytes: nothing of it may be read)
        free(d);
        d = nullptr;
    } else {
        memcpy(d, bytes.data(), n);
    }
    gzframe::Member m;
    gzframe::Header h;
    const gzframe::Kind kind = gzframe::member_at(d, n, 0, &m);
    const bool header = gzframe::parse_header(d, n, 0, &h);
    static const char *const names[] = {"none", "other", "bgzf", "forged"};
    printf("%zu %s size %zu isize %u header %d deflate_at %zu bgzf_size %zu magic %d\n", n, names[(int)kind], m.size, m.isize, (int)header,
           h.deflate_at, h.bgzf_size, (int)gzframe::magic_at(d, n, 0));
    free(d);
}

static void end_verdict(const std::vector<unsigned char> &bytes, size_t n, size_t at, uint32_t crc, uint32_t isize) {
    unsigned char *d = (unsigned char *)malloc(n ? n : 1);
    memcpy(d, bytes.data(), n);
    size_t next = 0;
    static const char *const names[] = {"truncated", "mismatch", "last", "member_follows"};
    const gzframe::End e = gzframe::member_end(d, n, at, crc, isize, &next);
    printf("%zu %s next %zu\n", n, names[(int)e], next);
    free(d);
}

int main(int argc, char **argv) {
    if (argc == 6 && strcmp(argv[1], "--end") == 0) {  // --end AT CRC ISIZE FILE: the end of a member whose trailer is at AT, per prefix
        FILE *f = fopen(argv[5], "rb");
        if (!f) return 2;
        std::vector<unsigned char> bytes;
        int c;
        while ((c = fgetc(f)) != EOF) bytes.push_back((unsigned char)c);
        fclose(f);
        const size_t at = (size_t)atoll(argv[2]);
        for (size_t n = at; n <= bytes.size(); ++n) end_verdict(bytes, n, at, (uint32_t)strtoul(argv[3], 0, 10), (uint32_t)strtoul(argv[4], 0, 10));
        return 0;
    }
    const bool prefixes = argc > 1 && strcmp(argv[1], "--prefixes") == 0;
    for (int a = prefixes ? 2 : 1; a < argc; ++a) {
        FILE *f = fopen(argv[a], "rb");
        if (!f) return 2;
        std::vector<unsigned char> bytes;
        int c;
        while ((c = fgetc(f)) != EOF) bytes.push_back((unsigned char)c);
        fclose(f);
        for (size_t n = prefixes ? 0 : bytes.size(); n <= bytes.size(); ++n) verdict(bytes, n);
    }
    return 0;
}
