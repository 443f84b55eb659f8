// report.h — `--report FILE`: what the filter did, as one JSON object — the reads of the input, the reads that were scored (children
// in place of their trimmed / split parents) and the reads that were kept, each summarised by the library (flx_summary: entries,
// bases, shortest, longest, median, N10..N90, histograms of length, mean quality and window quality; every field an integer).
// Not a flag of the reference, whose users run a statistics tool over the input and over the output instead.
// The three summaries are taken after the global stage and BEFORE the output pass — with several ranks they are collectives, and
// a rank that fails while writing must not leave the others alone in one — and the file is written by rank 0 once the run has
// succeeded: a run that ends with an error leaves the file as open_report_file (args.h) made it, empty.
#pragma once
#include <cstdio>
#include <string>

#include "run.h"

struct Report {
    std::string json;  // empty: no --report, or not rank 0
};

static void report_array(std::string &s, const char *key, const uint64_t *v, int n) {
    s += std::string("\"") + key + "\": [";
    for (int i = 0; i < n; ++i) s += (i ? ", " : "") + std::to_string(v[i]);
    s += "]";
}

static std::string report_summary(const struct flx_summary &m) {
    std::string s = "{\"n\": " + std::to_string(m.n) + ", \"bases\": " + std::to_string(m.bases) + ", \"min_length\": " + std::to_string(m.min_length) +
                    ", \"max_length\": " + std::to_string(m.max_length) + ", \"median_length\": " + std::to_string(m.median_length) + ", \"nx\": [";
    for (int i = 0; i < 9; ++i) s += (i ? ", " : "") + std::to_string(m.nx[i]);
    s += "], ";
    report_array(s, "len_count", m.len_count, FLX_SUMMARY_LEN_BINS); s += ", ";
    report_array(s, "len_bases", m.len_bases, FLX_SUMMARY_LEN_BINS); s += ", ";
    report_array(s, "mean_q_count", m.mean_q_count, FLX_SUMMARY_Q_BINS); s += ", ";
    report_array(s, "mean_q_bases", m.mean_q_bases, FLX_SUMMARY_Q_BINS); s += ", ";
    report_array(s, "window_q_count", m.window_q_count, FLX_SUMMARY_Q_BINS); s += ", ";
    report_array(s, "window_q_bases", m.window_q_bases, FLX_SUMMARY_Q_BINS);
    return s + "}";
}

// Every rank calls this at the same point, with its own share: three collectives in the same order everywhere.
// A rank on which a call fails before its first exchange (an allocation, a HIP error) leaves here alone and the others wait in the
// collective until rank 0's watchdog sees the early exit and ends the job (ranks.h) — the same exposure as exchange_totals.
static int summarise_for_report(const Run &run, const Pass1 &p, const flx_scores &res, const Reads2 &r2, Report &report) {
    if (!run.args.report_set) return kGoOn;
    const int global = run.world > 1;
    struct flx_summary input, scored, kept, excluded, low_complexity;
    if (flx_summary(run.ctx, p.lengths.size(), p.lengths.data(), res.mean_q, res.window_q, nullptr, global, &input) != FLX_OK ||
        flx_summary(run.ctx, r2.len.size(), r2.len.data(), r2.mean.data(), r2.window.data(), nullptr, global, &scored) != FLX_OK ||
        flx_summary(run.ctx, r2.len.size(), r2.len.data(), r2.mean.data(), r2.window.data(), r2.pass.data(), global, &kept) != FLX_OK)
        return run.fail("report");
    // --exclude: a fourth summary, the input reads the screen took (a collective like the other three)
    if (run.excluding() && flx_summary(run.ctx, p.lengths.size(), p.lengths.data(), res.mean_q, res.window_q, run.screen_excluded, global, &excluded) != FLX_OK)
        return run.fail("report");
    // --max_low_complexity: one more, the input reads the filter took, behind the screen's
    if (run.low_complexity() &&
        flx_summary(run.ctx, p.lengths.size(), p.lengths.data(), res.mean_q, res.window_q, run.complexity_flagged, global, &low_complexity) != FLX_OK)
        return run.fail("report");
    if (run.rank > 0) return kGoOn;
    double edges[51];
    flx_summary_q_edges(edges);
    std::string &s = report.json;
    s = "{\"version\": 1, \"q_edges\": [";
    for (int k = 0; k < 51; ++k) {
        char buf[40];
        snprintf(buf, sizeof buf, "%.17g", edges[k]);
        s += (k ? ", " : "") + std::string(buf);
    }
    s += "],\n \"input\": " + report_summary(input) + ",\n \"scored\": " + report_summary(scored) + ",\n \"kept\": " + report_summary(kept) +
         (run.excluding() ? ",\n \"excluded\": " + report_summary(excluded) : std::string()) +
         (run.low_complexity() ? ",\n \"low_complexity\": " + report_summary(low_complexity) : std::string()) + "}\n";
    return kGoOn;
}

static bool write_report(const Run &run, const Report &report) {
    if (report.json.empty()) return true;
    FILE *f = fopen(run.args.report.c_str(), "w");
    const bool ok = f && fwrite(report.json.data(), 1, report.json.size(), f) == report.json.size();
    if ((f && fclose(f) != 0) || !ok) {
        std::cerr << "Error: cannot write report file: " << run.args.report << "\n";
        return false;
    }
    return true;
}
