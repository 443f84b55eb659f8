// bam.h — unaligned BAM as the input of the long reads: detection, and the transcode of the inflated file into the FASTQ text
// everything downstream handles (the parser, pass 1, the output pass, --verbose, --report, --gzip, the ranks).  The reference has
// no BAM reader: its users put `samtools fastq` in front.  Included by main.cpp only (through run.h).
//
// A BAM input is a regular file that begins with a well-formed BGZF member whose first four bytes are "BAM\1".  Input::open
// inflates it like any gzip file, then bam_to_text replaces the bytes with their text:
//   FLX_CLI_GPU_BAM=1   through flx_bam_to_fastq (csrc/bam.hip); a device path that fails falls back to the host walk, silently;
//   FLX_CLI_GPU_BAM=0   the same csrc/bam_record.h walked on the host threads over record ranges.  The same bytes either way.
//   FLX_CLI_BAM_TIMING=1   one more stderr line: records, skipped records, `device` or `host`, milliseconds.
// Memory is O(inflated file + text): a BAM input is never streamed.  --bam without --trim / --split keeps the inflated file for
// the whole run (Input::keep_bam): the output pass writes the kept reads' original records out of it (output.h).
#pragma once
#include <chrono>
#include <functional>
#include <memory>

#include "../../include/filtlong_hip.h"
#include "../csrc/bam_record.h"

#include "fastx.h"

struct BamInput {
    std::function<flx_ctx *()> ctx;  // run.h: the process's context once it exists (null: none to be had); unset: no device
};
static BamInput g_bam;

// FLX_CLI_GPU_BAM: 0 by default — measured on one MI355X, the run with 1 (median 2.61 s on a 2 GB input) is not below the
// fastest run with 0 (2.05 s): the staging copies around the kernels cost more than the host walk
static bool bam_gpu_switch() {
    const char *e = getenv("FLX_CLI_GPU_BAM");
    return e && e[0] == '1';
}

static bool bam_detect(const unsigned char *file, size_t n) {
    uint64_t in_off[2], out_off[2], m = 0;
    if (flx_bgzf_index(file, n, 1, in_off, out_off, &m) != FLX_OK || m != 1 || out_off[1] < 4) return false;
    z_stream zs;
    memset(&zs, 0, sizeof zs);
    if (inflateInit2(&zs, 15 + 16) != Z_OK) return false;
    unsigned char first[4] = {0, 0, 0, 0};
    zs.next_in = const_cast<unsigned char *>(file);
    zs.avail_in = (uInt)in_off[1];
    zs.next_out = first;
    zs.avail_out = 4;
    const int rc = inflate(&zs, Z_SYNC_FLUSH);
    const bool got = (rc == Z_OK || rc == Z_STREAM_END) && zs.avail_out == 0;
    inflateEnd(&zs);
    return got && memcmp(first, "BAM\1", 4) == 0;
}

// The inflated file `data` (n bytes) as FASTQ text: false and a reason for a file that is truncated or malformed.
static bool bam_to_text(const char *data, size_t n, std::unique_ptr<char[]> &text, size_t &text_len, std::string &reason, uint64_t *header_len,
                        std::vector<uint64_t> *rec_at) {
    const auto t0 = std::chrono::steady_clock::now();
    const uint8_t *src = (const uint8_t *)data;
    uint64_t n_rec = 0, again = 0;
    int end = FLX_BAM_END;
    if (flx_bam_index(src, n, UINT64_MAX, nullptr, &n_rec, &end) != FLX_OK) { reason = "index"; return false; }
    if (end == FLX_BAM_HEADER) reason = "bad header";
    else if (end == FLX_BAM_TRUNCATED) reason = n_rec == 0 && n < 12 ? "truncated header" : "truncated inside record " + std::to_string(n_rec) + " (or inside the header)";
    else if (end == FLX_BAM_MALFORMED) reason = "record " + std::to_string(n_rec) + " is malformed";
    if (end != FLX_BAM_END) return false;
    std::vector<uint64_t> rec_off(n_rec + 1);
    if (flx_bam_index(src, n, n_rec, rec_off.data(), &again, &end) != FLX_OK || again != n_rec) { reason = "index"; return false; }
    // record ranges for the host threads: their text sizes first (one cache line per record), so the text is allocated once
    const size_t parts = (size_t)std::min<uint64_t>(std::max<uint64_t>(n_rec, 1), (uint64_t)host_threads() * 8);
    std::vector<uint64_t> first(parts + 1), at(parts + 1, 0), skipped(parts, 0);
    for (size_t i = 0; i <= parts; ++i) first[i] = n_rec / parts * i + std::min<uint64_t>(i, n_rec % parts);
    parallel_for(parts, [&](size_t i) { at[i + 1] = bam::text_bytes_host(src, rec_off.data(), first[i], first[i + 1], &skipped[i]); });
    uint64_t n_skipped = 0;
    for (size_t i = 0; i < parts; ++i) { at[i + 1] += at[i]; n_skipped += skipped[i]; }
    text_len = (size_t)at[parts];
    text.reset(new char[text_len ? text_len : 1]);
    bool device = false;
    if (bam_gpu_switch() && g_bam.ctx && n_rec > 0) {
        if (flx_ctx *ctx = g_bam.ctx()) {
            uint64_t len = 0, sk = 0, bad = 0;
            device = flx_bam_to_fastq(ctx, src, n, rec_off.data(), n_rec, 0, text.get(), text_len, nullptr, &len, &sk, &bad) == FLX_OK &&
                     len == text_len && bad == n_rec;
        }
    }
    if (!device) parallel_for(parts, [&](size_t i) { bam::emit_records_host(src, rec_off.data(), first[i], first[i + 1], (uint8_t *)text.get() + at[i]); });
    *header_len = rec_off[0];
    if (rec_at) {  // (--bam, reads that go out whole: the record of every text record; one cache line per record, as above)
        rec_at->clear();
        rec_at->reserve((size_t)(n_rec - n_skipped));
        for (uint64_t k = 0; k < n_rec; ++k) {
            bam::Rec r;
            if (bam::read_record(src, rec_off[k + 1], rec_off[k], r) == bam::REC_OK && bam::has_text(r)) rec_at->push_back(rec_off[k]);
        }
    }
    if (const char *e = getenv("FLX_CLI_BAM_TIMING"); e && e[0] == '1')
        fprintf(stderr, "[bam] %llu record(s), %llu skipped, %s, %.3f ms\n", (unsigned long long)n_rec, (unsigned long long)n_skipped,
                device ? "device" : "host", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    return true;
}

static const BamHooks kBamHooks = {bam_detect, bam_to_text};
