// filtlong-amd — C++ host of the MI355X-native Filtlong hot path: same command line, same stdout FASTQ/FASTA,
// same stderr lines and exit codes as the reference binary, with the per-read scoring and the global rank/cut
// done on the GPU through the C ABI (include/filtlong_hip.h).
//
// What this file mirrors of the reference (rrwick/Filtlong v0.3.1, paths relative to its root):
//   arguments       src/arguments.cpp:28-393  flags, unit suffixes, validation order and messages
//   input parsing   src/kseq.h:176-224         FASTA/FASTQ records, multi-line, "\r\n", gz via zlib
//   orchestration   src/main.cpp:37-321        sections printed to stderr, reads2 gather, output order
//   formatting      src/misc.cpp:24-49         2-decimal doubles, locale-grouped integers
// Differences by design: a plain file is mapped and parsed once (the reference parses it twice, main.cpp:70-127 and
// 264-313), a gzip file is streamed block by block (gzblocks.h); scoring is batched and streamed (flx_pipeline_*) instead of
// one Read object per record; ranks (one process per GPU) share the global stage through the library's communicator.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#include <unistd.h>

#include "../../include/filtlong_hip.h"

#include "args.h"
#include "format.h"
#include "output.h"
#include "parse_only.h"
#include "pass1.h"
#include "ranks.h"
#include "reference.h"
#include "report.h"
#include "run.h"
#include "verbose.h"

// ---- reads2: children replace their parents in place (src/main.cpp:138-147) -----------------------------
static int gather_reads2(const Run &run, const Pass1 &p, const flx_scores &res, Reads2 &r2) {
    // the gather itself is the library's (flx_reads2_gather): values in reads2 order + where every entry came from
    const uint64_t n = p.lengths.size(), cap2 = n + res.n_children;
    r2.mean.resize(cap2); r2.window.resize(cap2); r2.len.resize(cap2); r2.pass.resize(cap2);
    std::vector<uint32_t> parent2(cap2);
    std::vector<int64_t> child2(cap2);
    uint64_t n2_gathered = 0;
    if (flx_reads2_gather(run.ctx, n, p.lengths.data(), &res, cap2, r2.mean.data(), r2.window.data(), r2.len.data(), r2.pass.data(),
                          parent2.data(), child2.data(), &n2_gathered) != FLX_OK)
        return run.fail("reads2 gather");
    r2.mean.resize(n2_gathered); r2.window.resize(n2_gathered); r2.len.resize(n2_gathered); r2.pass.resize(n2_gathered);
    r2.reads.reserve(n2_gathered);
    const int32_t *c_ranges = res.child_ranges;
    for (uint64_t j = 0; j < n2_gathered; ++j) {
        const uint64_t i = parent2[j];
        if (child2[j] < 0) {
            r2.reads.push_back({p.lo_rec + i, 0, p.lengths[i], false, std::string(p.names[i])});
        } else {
            const int s0 = c_ranges[2 * child2[j]], e0 = c_ranges[2 * child2[j] + 1];
            r2.reads.push_back({p.lo_rec + i, s0, e0, true, std::string(p.names[i]) + "_" + std::to_string(s0 + 1) + "-" + std::to_string(e0)});  // read.cpp:135-136
        }
    }
    for (auto &o : r2.reads) r2.longest_name = std::max(r2.longest_name, o.name.size());
    return kGoOn;
}

// totals over all ranks (one rank: the local values), and the line of src/main.cpp:155-166
static int exchange_totals(const Run &run, const Pass1 &p, const flx_scores &res, Reads2 &r2) {
    const Args &args = run.args;
    const int rank = run.rank, world = run.world;
    long long after_total = 0;
    for (auto v : r2.len) after_total += v;
    r2.n_total = r2.reads.size();
    uint64_t excluded_reads = 0, excluded_bases = 0;  // --exclude: the input reads the screen took
    if (run.screen_excluded)
        for (size_t i = 0; i < p.lengths.size(); ++i)
            if (run.screen_excluded[i]) { ++excluded_reads; excluded_bases += (uint64_t)p.lengths[i]; }
    uint64_t lowc_reads = 0, lowc_bases = 0;  // --max_low_complexity: the input reads the filter took
    if (run.complexity_flagged)
        for (size_t i = 0; i < p.lengths.size(); ++i)
            if (run.complexity_flagged[i]) { ++lowc_reads; lowc_bases += (uint64_t)p.lengths[i]; }
    uint64_t split_reads = 0;  // --split_adapters: the input reads that went on as two children or more
    if (args.split_adapters && res.child_offsets)
        for (size_t i = 0; i < p.lengths.size(); ++i)
            if (res.child_offsets[i + 1] - res.child_offsets[i] >= 2) ++split_reads;
    if (world > 1) {
        const size_t lowc_at = 2 * (size_t)world + 1 + (run.excluding() ? 2 : 0);
        std::vector<uint64_t> sums(lowc_at + (run.low_complexity() ? 2 : 0) + (args.split_adapters ? 1 : 0), 0);
        if (args.split_adapters) sums.back() = split_reads;
        if (run.excluding()) { sums[2 * (size_t)world + 1] = excluded_reads; sums[2 * (size_t)world + 2] = excluded_bases; }
        if (run.low_complexity()) { sums[lowc_at] = lowc_reads; sums[lowc_at + 1] = lowc_bases; }
        sums[rank] = r2.reads.size();
        sums[world] = (uint64_t)after_total;
        sums[(size_t)world + 1 + rank] = r2.longest_name;  // (the --verbose table pads every name to the longest of ALL reads2, main.cpp:199-201)
        if (flx_comm_sum_u64(run.ctx, sums.data(), sums.size()) != FLX_OK) return run.fail("exchange");
        r2.n_total = 0;
        for (int r = 0; r < world; ++r) { r2.n_total += sums[r]; r2.longest_name = std::max<size_t>(r2.longest_name, sums[(size_t)world + 1 + r]); }
        after_total = (long long)sums[world];
        if (run.excluding()) { excluded_reads = sums[2 * (size_t)world + 1]; excluded_bases = sums[2 * (size_t)world + 2]; }
        if (run.low_complexity()) { lowc_reads = sums[lowc_at]; lowc_bases = sums[lowc_at + 1]; }
        if (args.split_adapters) split_reads = sums.back();
        if (args.verbose && rank == 0) {
            if (!print_verbose_parts(run, "vblocks")) return 1;
            std::cerr << "\n";
        }
    }
    if (run.excluding() && rank == 0)
        std::cerr << "  excluded by reference: " << int_to_string((long long)excluded_reads) << " reads (" << int_to_string((long long)excluded_bases) << " bp)\n";
    if (run.low_complexity() && rank == 0)
        std::cerr << "  low complexity: " << int_to_string((long long)lowc_reads) << " reads (" << int_to_string((long long)lowc_bases) << " bp)\n";
    if ((args.trim || args.split_set || args.split_window_q_set || args.trim_adapters_set || args.trim_ends_q_set) && rank == 0) {  // src/main.cpp:155-166 (--split_window_q: "after splitting")
        if (args.split_adapters) std::cerr << "  split at adapters: " << int_to_string((long long)split_reads) << " reads\n";
        if (args.trim_adapters_set) std::cerr << "  after adapter trimming: ";
        else if (args.trim_ends_q_set) std::cerr << "  after quality trimming: ";
        else if (args.trim && args.split_set) std::cerr << "  after trimming and splitting: ";
        else if (args.trim) std::cerr << "  after trimming: ";
        else std::cerr << "  after splitting: ";
        std::cerr << int_to_string((long long)r2.n_total) << " reads (" << int_to_string(after_total) << " bp)\n";
    }
    if (rank == 0) std::cerr << "\n";
    return kGoOn;
}

// ---- global stage (src/main.cpp:169-261) ---------------------------------------------------------------
static int rank_and_cut(const Run &run, const Pass1 &p, Reads2 &r2, flx_cut_report &rep) {
    const Args &args = run.args;
    memset(&rep, 0, sizeof rep);
    if (r2.n_total == 0 && !args.target_bases_set && !args.keep_percent_set) return kGoOn;
    const auto fn = run.world > 1 ? flx_rank_and_cut_comm : flx_rank_and_cut;
    if (fn(run.ctx, r2.reads.size(), r2.mean.data(), r2.window.data(), r2.len.data(), r2.pass.data(), args.length_weight, args.mean_q_weight,
           args.window_q_weight, args.target_bases_set, args.target_bases, args.keep_percent_set, args.keep_percent, p.total_bases, nullptr,
           &rep) != FLX_OK)
        return run.fail("rank and cut");
    return kGoOn;
}

static void print_cut_report(const Run &run, const flx_cut_report &rep) {
    if ((!run.args.target_bases_set && !run.args.keep_percent_set) || run.rank > 0) return;
    std::cerr << "Filtering long reads\n";
    std::cerr << "  target: " << int_to_string(rep.target_bases) << " bp\n";
    if (rep.outcome == FLX_CUT_NOT_ENOUGH) std::cerr << "  not enough reads to reach target\n";
    else if (rep.outcome == FLX_CUT_ALREADY_BELOW) std::cerr << "  reads already fall below target after filtering\n";
    else std::cerr << "  keeping " << int_to_string(rep.kept_bases) << " bp\n";
    std::cerr << "\n";
}

// The output is complete.  Unpinning the staging buffers, shutting the HIP runtime down and unmapping the input is work the
// kernel does faster when the process simply ends (0.5-0.9 s of 1.3-2.7 s on 2-10 GB inputs): flush and leave, unless a
// clean teardown is asked for (FLX_CLI_CLEAN_EXIT=1, the timing report, or ranks to reap).
static int leave(Run &run, Scorer &scorer, const Report &report) {
    const bool clean_exit = getenv("FLX_CLI_CLEAN_EXIT") != nullptr || run.timing;
    if (clean_exit) {
        scorer.destroy();
        run.stage("pipeline teardown");
        if (run.kmers) flx_kmerset_destroy(run.kmers);
        run.destroy_exclude();
        if (run.adapters) flx_adapters_destroy(run.adapters);
        g_gpu_inflater.destroy();
        flx_ctx_destroy(run.ctx);
        run.stage("context teardown");
    }
    if (!g_job.finish()) { std::cerr << "Error: a rank failed\n"; return 1; }
    run.print_wall_clock("returns");
    if (run.rank == 0) std::cerr << "\n";
    bool flushed = fflush(stdout) == 0 && !ferror(stdout);
    if (flushed) flushed = write_report(run, report);  // (--report: only a run that succeeded leaves more than an empty file)
    fflush(stderr);
    if (!clean_exit) _exit(flushed ? 0 : 1);
    return flushed ? 0 : 1;
}

// The FLX_CLI_* environment variables this binary reads (test hooks and tuning knobs, README.md); any other FLX_CLI_* name is an
// error — a mistyped switch must not be ignored silently.  (The library checks the rest of the FLX_* names: flx_ctx_create.)
static int check_cli_environment() {
    static const char *const known[] = {
        "FLX_CLI_BAM_TIMING", "FLX_CLI_BLOCK_BYTES", "FLX_CLI_BLOCK_MB", "FLX_CLI_CHUNK_BYTES", "FLX_CLI_CHUNK_MB", "FLX_CLI_CLEAN_EXIT", "FLX_CLI_FORCE_STREAM",
        "FLX_CLI_FAIL_WRITE_RANK", "FLX_CLI_GPU_BAM", "FLX_CLI_GPU_INFLATE", "FLX_CLI_GPU_INFLATE_OUTPUT", "FLX_CLI_INFLATE_THREADS", "FLX_CLI_NO_STREAM", "FLX_CLI_ORDERED_OUTPUT", "FLX_CLI_PARALLEL_PARSE_MIN", "FLX_CLI_PARSE_ONLY",
        "FLX_CLI_PINFLATE", "FLX_CLI_PINFLATE_AHEAD_MB", "FLX_CLI_PINFLATE_CHUNK", "FLX_CLI_PINFLATE_MIN", "FLX_CLI_PINFLATE_TIMING",
        "FLX_CLI_RANK_RANGES", "FLX_CLI_RANK_STREAM", "FLX_CLI_REF_BATCH_BYTES", "FLX_CLI_SPAN_BYTES", "FLX_CLI_THREADS", "FLX_CLI_TIMING",
    };
    for (char **e = environ; e && *e; ++e) {
        if (strncmp(*e, "FLX_CLI_", 8) != 0) continue;
        const char *eq = strchr(*e, '=');
        const std::string name(*e, eq ? (size_t)(eq - *e) : strlen(*e));
        bool ok = false;
        for (const char *k : known) ok = ok || name == k;
        if (!ok) {
            std::cerr << "Error: unknown environment variable " << name << " (the FLX_CLI_* switches are listed in README.md)\n";
            return 1;
        }
    }
    for (const char *name : {"FLX_CLI_GPU_BAM", "FLX_CLI_GPU_INFLATE", "FLX_CLI_GPU_INFLATE_OUTPUT"})
        if (const char *e = getenv(name))
            if (strcmp(e, "0") != 0 && strcmp(e, "1") != 0) {
                std::cerr << "Error: " << name << " must be 0 or 1\n";
                return 1;
            }
    return 0;
}

int main(int argc, char **argv) {
    Args args;
    const ParsingResult pr = parse_args(argc, argv, args);
    if (pr == BAD) return 1;
    if (pr == HELP) return 0;
    if (pr == VERSION) { std::cout << "Filtlong v" << PROGRAM_VERSION << "\n"; return 0; }
    if (const int bad_env = check_cli_environment()) return bad_env;
    if (const char *po = getenv("FLX_CLI_PARSE_ONLY")) return parse_only(args.input_reads, po);
    if (!open_report_file(args)) return 1;  // --report: created or emptied here, before any work

    // ---- ranks: one process per GPU (north_star / SURVEY §8e; ranks.h) — under a launcher, or forked here by --gpus N ----
    Run run(args);
    std::string id_file;
    int id_pipe = -1;  // --gpus: the read end of this rank's pipe from rank 0
    if (const int rc = start_ranks(run, id_file, id_pipe); rc != kGoOn) return rc;
    JobGuard job_guard;  // rank 0 of --gpus: whatever way main() is left, no child and no part file stays behind
    if (run.rank < 0 || run.rank >= run.world) { std::cerr << "Error: RANK " << run.rank << " outside WORLD_SIZE " << run.world << "\n"; return 1; }
    if (args.gpus > 1 && run.world > 1 && id_file.empty()) g_shared_out = dup(1);  // (forked ranks share the job's stdout: see the output pass)
    if (run.rank > 0) {  // rank 0 speaks for the job
        if (!freopen("/dev/null", "w", stderr)) return 1;
        if (!freopen("/dev/null", "w", stdout)) return 1;
    }

    std::cerr << "\n";
    run.timing = getenv("FLX_CLI_TIMING") != nullptr;
    run.t0 = now_s();
    run.print_wall_clock("reached");
    if (const int rc = run.create_context(); rc != kGoOn) return rc;  // (on a second thread where nothing needs it yet: run.h)
    if (run.world > 1)
        if (const int rc = exchange_communicator_id(run, id_file, id_pipe); rc != kGoOn) return rc;
    run.arm_inflater();
    run.arm_bam();
    run.stage("context");

    // ---- reference 16-mers (src/main.cpp:51-59, src/kmers.cpp:50-72) --------------------------------------
    if (const int rc = build_reference_set(run); rc != kGoOn) return rc;
    if (const int rc = build_exclude_set(run); rc != kGoOn) return rc;  // --exclude: the contaminant's set, on every rank
    if (const int rc = build_adapters(run); rc != kGoOn) return rc;    // --trim_adapters: the adapters' patterns, on every rank
    run.stage("reference 16-mers");

    // ---- pass 1: parse, checks (src/main.cpp:63-130) -----------------------------------------------------
    if (!args.verbose) std::cerr << "Scoring long reads\n";
    ReadsInput in;
    if (const int rc = open_reads_input(run, in); rc != kGoOn) return rc;
    if (const int rc = count_pass(run, in); rc != kGoOn) return rc;
    Pass1 p;
    Scorer scorer(run, in.streamed);  // (declared behind `run`: the pipeline is destroyed before the context's thread is joined)
    if (in.streamed) {
        if (const int rc = pass1_streamed(run, in, p, scorer); rc != kGoOn) return rc;
    } else {
        bool ranged = false;
        if (const int rc = pass1_rank_range(run, in, p, scorer, ranged); rc != kGoOn) return rc;
        if (!ranged)
            if (const int rc = pass1_mapped(run, in, p, scorer); rc != kGoOn) return rc;
    }
    if (!args.verbose) print_progress(p.n_records, p.total_bases);
    if (!args.verbose) std::cerr << "\n";  // verbose: after the per-read blocks, as in main.cpp:110-129
    flx_scores res;
    if (const int rc = scorer.finish(res, p.lengths.size()); rc != kGoOn) return rc;
    if (run.timing) fprintf(stderr, "[timing] %llu chunk(s) of <= %llu MiB\n", (unsigned long long)scorer.n_chunks, (unsigned long long)(scorer.chunk_bytes >> 20));
    run.stage("pack + H2D + score (streamed)");

    // ---- reads2: children replace their parents in place (src/main.cpp:138-147) -----------------------------
    Reads2 r2;
    if (const int rc = gather_reads2(run, p, res, r2); rc != kGoOn) return rc;
    if (const int rc = print_verbose_blocks(run, p, res); rc != kGoOn) return rc;
    if (const int rc = exchange_totals(run, p, res, r2); rc != kGoOn) return rc;

    // ---- global stage (src/main.cpp:169-261) ---------------------------------------------------------------
    flx_cut_report rep;
    if (const int rc = rank_and_cut(run, p, r2, rep); rc != kGoOn) return rc;
    if (const int rc = print_verbose_table(run, r2, rep); rc != kGoOn) return rc;
    print_cut_report(run, rep);
    run.stage("rank and cut");
    Report report;  // --report: summarised here, in front of the output pass (collectives with several ranks), written on the way out
    if (const int rc = summarise_for_report(run, p, res, r2, report); rc != kGoOn) return rc;
    if (args.report_set) run.stage("report");

    // ---- output in input order (src/main.cpp:263-313) -----------------------------------------------------
    Output out;
    const Emitter em(r2, p);
    if (const int rc = begin_output(run, out, in, p, em); rc != kGoOn) return rc;
    if (const int rc = in.streamed ? write_output_streamed(run, in, p, em, out) : write_output_mapped(run, in, p, em, out); rc != kGoOn) return rc;
    if (const int rc = finish_output(run, out, em); rc != kGoOn) return rc;
    run.stage("output");

    return leave(run, scorer, report);
}
