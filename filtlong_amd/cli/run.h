// run.h — the state the stages of main() hand on: `Run` (what is fixed once start-up is over), `Pass1` (what survives pass 1 per
// record), `Reads2` (the reads after trimming and splitting), and the small rules more than one stage uses.
#pragma once
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <iostream>
#include <string>
#include <string_view>
#include <thread>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "../../include/filtlong_hip.h"

#include "args.h"
#include "bam.h"
#include "fastx.h"
#include "gzblocks.h"

// What every stage returns: kGoOn, or the exit status to leave main() with (0 as well: a rank > 0 leaves quietly on an input error).
constexpr int kGoOn = -1;

static double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

struct Run {
    const Args &args;
    int rank = 0, world = 1;   // multi-GPU: one process per GPU (RANK / WORLD_SIZE, or forked by --gpus N)
    std::string part_prefix;   // where the ranks leave their parts of the output
    bool timing = false;
    double t0 = 0;
    // The context (HIP runtime start-up, ~0.1 s) is created on a second thread while the first one maps, parses and checks the input,
    // when nothing needs it before the scoring: one rank, no reference 16-mers to build.
    flx_ctx *ctx = nullptr;
    int ctx_rc = FLX_OK;
    std::thread ctx_thread;
    flx_kmerset *kmers = nullptr;
    bool kmers_empty = true;
    flx_kmerset *exclude = nullptr;            // --exclude: the contaminant's 16-mers (reference.h: build_exclude_set)
    flx_screenset *exclude_hash = nullptr;     // --exclude_k 17..31: the contaminant's canonical K-mers instead (one of the two)
    int exclude_k = 16;                        // the K of whichever set was built
    bool excluding() const { return exclude != nullptr || exclude_hash != nullptr; }
    int set_pipeline_screen(flx_pipeline *pipe) const {  // the pipeline screens every chunk against whichever set was built
        return exclude_hash ? flx_pipeline_set_screenset(pipe, exclude_hash, args.exclude_percent) : flx_pipeline_set_screen(pipe, exclude, args.exclude_percent);
    }
    void destroy_exclude() {
        if (exclude) flx_kmerset_destroy(exclude);
        if (exclude_hash) flx_screenset_destroy(exclude_hash);
        exclude = nullptr;
        exclude_hash = nullptr;
    }
    const uint32_t *screen_hits = nullptr;     // ... and, once the scores are in, every read's hits and whether it was excluded
    const uint8_t *screen_excluded = nullptr;  // (owned by the pipeline; this rank's reads in submission order)
    bool low_complexity() const { return args.max_low_complexity_set; }  // --max_low_complexity: the pipeline also counts every read's bad windows
    const uint32_t *complexity_bad = nullptr;  // ... and, once the scores are in, every read's bad windows and whether it was flagged
    const uint8_t *complexity_flagged = nullptr;  // (owned by the pipeline; this rank's reads in submission order)
    flx_adapters *adapters = nullptr;          // --trim_adapters: the patterns (reference.h: build_adapters) ...
    std::vector<std::string> adapter_names;    // ... the names of their sequences (pattern p belongs to sequence p / 2) ...
    const uint32_t *adapter_keys = nullptr;    // ... and, once the scores are in, every read's head and tail key (owned by the pipeline)
    const uint32_t *endtrim_cuts = nullptr;    // --trim_ends_q: once the scores are in, every read's head and tail cut (owned by the pipeline)
    flx_params prm;

    explicit Run(const Args &a) : args(a) {
        memset(&prm, 0, sizeof prm);
        prm.window_size = a.window_size;  // (already narrowed to the reference's int by parse_args)
        prm.min_length_set = a.min_length_set; prm.min_length = a.min_length;
        prm.max_length_set = a.max_length_set; prm.max_length = a.max_length;
        prm.min_mean_q_set = a.min_mean_q_set; prm.min_mean_q = a.min_mean_q;
        prm.min_window_q_set = a.min_window_q_set; prm.min_window_q = a.min_window_q;
        prm.trim = a.trim; prm.split_set = a.split_set; prm.split = a.split;
    }
    Run(const Run &) = delete;
    ~Run() { if (ctx_thread.joinable()) ctx_thread.join(); }

    void print_wall_clock(const char *what) const {
        if (!timing) return;
        struct timespec ts;
        clock_gettime(CLOCK_REALTIME, &ts);
        fprintf(stderr, "[timing] main() %s at wall clock %.3f\n", what, ts.tv_sec % 100000 + ts.tv_nsec * 1e-9);
    }
    void stage(const char *what) {  // FLX_CLI_TIMING=1: per-stage wall clock + resident memory on stderr (not part of the reference surface)
        if (!timing) return;
        const double t = now_s();
        long anon_kb = 0, file_kb = 0, hwm_kb = 0;
        if (FILE *f = fopen("/proc/self/status", "r")) {  // RssAnon = what the process owns; RssFile = resident pages of the mapped input
            char line[256];
            while (fgets(line, sizeof line, f)) {
                sscanf(line, "RssAnon: %ld kB", &anon_kb);
                sscanf(line, "RssFile: %ld kB", &file_kb);
                sscanf(line, "VmHWM: %ld kB", &hwm_kb);
            }
            fclose(f);
        }
        fprintf(stderr, "[timing] %-30s %8.3f s   RssAnon %7ld MiB  RssFile %7ld MiB  VmHWM %7ld MiB\n", what, t - t0, anon_kb >> 10,
                file_kb >> 10, hwm_kb >> 10);
        t0 = now_s();
    }
    int fail(const char *what) const {
        std::cerr << "Error: " << what << ": " << flx_last_error(ctx) << "\n";
        return 1;
    }
    int create_context() {
        const char *dev = getenv("FLX_DEVICE");
        int ordinal = dev ? atoi(dev) : 0;
        if (!dev && world > 1) ordinal = getenv("LOCAL_RANK") ? atoi(getenv("LOCAL_RANK")) : rank;
        if (world == 1 && !args.assembly_set && args.short_reads.empty() && !args.exclude_set && !timing) {
            ctx_thread = std::thread([this, ordinal] { ctx_rc = flx_ctx_create(ordinal, &ctx); });
        } else if (flx_ctx_create(ordinal, &ctx) != FLX_OK) {
            std::cerr << "Error: " << flx_last_error(nullptr) << "\n";
            return 1;
        }
        return kGoOn;
    }
    bool ready() {  // before the first use of `ctx`
        if (ctx_thread.joinable()) ctx_thread.join();
        if (ctx_rc != FLX_OK) {
            std::cerr << "Error: " << flx_last_error(nullptr) << "\n";
            ctx_rc = FLX_OK;  // reported once
            return false;
        }
        return ctx != nullptr;
    }
    // FLX_CLI_GPU_INFLATE=1: BGZF input (the reads, the count pass, the -a / -1 / -2 references) is inflated on the device, by one
    // object per process.  It is created when the first BGZF input is opened (gzblocks.h), behind the context, which that input then
    // waits for; nothing else does.  A context or an object that cannot be had is no error here: the input is zlib's, as with the
    // switch at 0, and whoever needs the context next reports it.  0, the default: zlib on the host threads.
    // FLX_CLI_GPU_INFLATE_OUTPUT=1 sends the output pass's re-inflation (inflate_range) through the same object.
    static bool switch_on(const char *e) { return e && e[0] == '1'; }
    void arm_inflater() {
        if (!switch_on(getenv("FLX_CLI_GPU_INFLATE"))) return;
        g_gpu_inflater.output_pass = switch_on(getenv("FLX_CLI_GPU_INFLATE_OUTPUT"));
        g_gpu_inflater.make = [this]() -> flx_bgzf * {
            if (ctx_thread.joinable()) ctx_thread.join();
            flx_bgzf *z = nullptr;
            if (ctx_rc != FLX_OK || !ctx) return nullptr;
            if (flx_bgzf_create(ctx, 16u << 20, (unsigned)std::min<size_t>(host_threads(), 16), &z) != FLX_OK) return nullptr;
            return z;
        };
    }
    // FLX_CLI_GPU_BAM=1: a BAM input is turned into text on the device (bam.h), which then waits for the context like the inflater
    void arm_bam() {
        g_bam.ctx = [this]() -> flx_ctx * {
            if (ctx_thread.joinable()) ctx_thread.join();
            return ctx_rc == FLX_OK ? ctx : nullptr;
        };
    }
    // a rank's file in the job's private directory: its "part" of the output, its "vblocks" and "vtable" of --verbose
    std::string part_path(const char *kind, int r) const { return part_prefix + "." + kind + std::to_string(r); }
};

// A rank's contiguous share of n records of file order, by COUNT: records [lo, lo + cnt).
struct Share { uint64_t lo, cnt; };
static Share rank_share(uint64_t n, int world, int rank) {
    return {n / (uint64_t)world * (uint64_t)rank + std::min<uint64_t>((uint64_t)rank, n % (uint64_t)world),
            n / (uint64_t)world + ((uint64_t)rank < n % (uint64_t)world ? 1 : 0)};
}

// A record that is a header and nothing else (no sequence, no '+' line; kseq returns it with length 0, src/kseq.h:206-213) prints
// oddly in the reference's FASTQ output: src/main.cpp:279 sends the C string seq->qual.s, and kseq has only reset that buffer's
// LENGTH — the quality string of the last record in front of it that had a '+' line comes out again.  With no such record the
// pointer is null, std::cout goes bad and nothing at all is written from there on.  Both are reproduced: the string to print
// is noted here, in file order; the stream's death is decided in the output pass (only a record that passes prints).
struct HeaderOnly {
    std::unordered_map<uint64_t, std::string> stale_qual;  // header-only record -> the quality string the reference prints for it
    std::unordered_set<uint64_t> null_qual;                 // header-only records in front of the first '+' line
    bool have_plus = false;
    View last_plus_qual;            // quality of the last record with a '+' line in the current batch ...
    std::string last_plus_stash;    // ... or, from an earlier block of a streamed input, a copy of it
    bool last_plus_in_batch = false;
    void note(const Record &r, uint64_t index) {
        if (r.is_fastq) {
            have_plus = true;
            last_plus_qual = r.qual;
            last_plus_in_batch = true;
        } else if (r.seq.empty()) {
            if (!have_plus) null_qual.insert(index);
            else stale_qual.emplace(index, last_plus_in_batch ? std::string(last_plus_qual.p, last_plus_qual.n) : last_plus_stash);
        }
    }
    void end_of_block() {  // the block's memory goes away
        if (!last_plus_in_batch) return;
        last_plus_stash.assign(last_plus_qual.p, last_plus_qual.n);
        last_plus_in_batch = false;
    }
};

// what survives pass 1 for this rank's records: lengths and names (views into the mapped input, or copies when streaming)
struct Pass1 {
    Parsed kept;                          // the single batch of a mapped / in-memory input
    std::vector<int32_t> lengths;
    std::vector<std::string_view> names;
    std::deque<std::string> name_arena;
    uint64_t lo_rec = 0;                  // first record of this rank's contiguous block of file order
    uint64_t n_records = 0;               // of the whole file
    long long total_bases = 0, last_progress = 0;
    bool any_fasta = false, any_fastq = false;
    UnitIndex units;                      // streamed input: the record-aligned pieces the output pass inflates concurrently
    HeaderOnly header_only;
};

// reads2: children replace their parents in place (src/main.cpp:138-147)
struct Reads2 {
    struct Out { uint64_t rec; int start, end; bool child; std::string name; };
    std::vector<Out> reads;
    std::vector<double> mean, window;
    std::vector<int32_t> len;
    std::vector<uint8_t> pass;
    size_t longest_name = 0;
    uint64_t n_total = 0;  // reads2 of all ranks (one rank: reads.size())
};
