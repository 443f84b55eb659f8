// verbose.h — what --verbose adds to stderr: a block per read (src/read.cpp:169-194), the table of scores (src/main.cpp:199-214), and
// with several ranks the files through which rank r > 0 hands its blocks and rows to rank 0.
#pragma once
#include <cmath>
#include <fstream>

#include "format.h"
#include "run.h"

// Read::print_verbose_read_info for reads [0, n_first) (src/read.cpp:169-194), in file order like the pass-1 loop (main.cpp:110-111)
static void print_read_blocks(std::ostream &os, const Run &run, const Pass1 &p, const flx_scores &res, uint64_t n_first) {
    const Args &args = run.args;
    const std::vector<int32_t> &lengths = p.lengths;
    const double *mean_q = res.mean_q, *window_q = res.window_q, *c_mean = res.child_mean_q, *c_window = res.child_window_q;
    const int32_t *c_ranges = res.child_ranges;
    const uint64_t *child_off = res.child_offsets;
    const uint64_t n = n_first;
    for (uint64_t i = 0; i < n; ++i) {
        const std::string_view rname = p.names[i];
        os << "\n" << rname << "\n";
        os << "            length = " << pad(std::to_string(lengths[i]), 11) << "mean quality = " << double_to_string(mean_q[i])
                  << "      window quality = " << double_to_string(window_q[i]) << "\n";
        const uint64_t a = child_off[i], b = child_off[i + 1];
        // m_bad_ranges (read.cpp:86-117): disjoint, non-adjacent and sorted, so with children they are exactly the gaps the
        // children leave in [0, L); without children the only possibility is the whole read (no covered base at all and
        // at least --split long)
        std::vector<std::pair<int, int>> bad;
        if (a != b) {
            int from = 0;
            for (uint64_t k = a; k < b; ++k) {
                if (c_ranges[2 * k] > from) bad.push_back({from, c_ranges[2 * k]});
                from = c_ranges[2 * k + 1];
            }
            if (from < lengths[i]) bad.push_back({from, lengths[i]});
        } else if (!run.kmers_empty && args.split_set && res.first[i] == -1 && lengths[i] > 0 && lengths[i] >= args.split) {
            bad.push_back({0, lengths[i]});
        } else if (args.split_window_q_set && res.first[i] == -1 && lengths[i] > 0) {  // --split_window_q: every base lies in a bad window
            bad.push_back({0, lengths[i]});
        } else if (run.adapter_keys && res.first[i] == -1 && lengths[i] > 0) {  // --trim_adapters: the two cuts leave nothing
            bad.push_back({0, lengths[i]});
        } else if (run.endtrim_cuts && res.first[i] == -1 && lengths[i] > 0) {  // --trim_ends_q: the two cuts leave nothing
            bad.push_back({0, lengths[i]});
        }
        if (!bad.empty()) {
            os << "        bad ranges = ";
            for (size_t k = 0; k < bad.size(); ++k) os << bad[k].first << "-" << bad[k].second << (k + 1 < bad.size() ? ", " : "");
            os << "\n";
        }
        if (a != b) {
            os << "      child ranges = ";
            for (uint64_t k = a; k < b; ++k) os << c_ranges[2 * k] << "-" << c_ranges[2 * k + 1] << (k + 1 < b ? ", " : "");
            os << "\n";
        }
        if (run.adapter_keys) {  // --trim_adapters: the cut lengths and whose adapter reached furthest, behind the lines of the parent's block
            const uint32_t kh = run.adapter_keys[2 * i], kt = run.adapter_keys[2 * i + 1];
            os << "          adapters = start " << (kh >> 8) << " (" << (kh ? run.adapter_names[(kh & 255u) >> 1] : std::string("none")) << "), end "
               << (kt >> 8) << " (" << (kt ? run.adapter_names[(kt & 255u) >> 1] : std::string("none")) << ")\n";
            if (args.split_adapters) {  // --split_adapters: the adapter occurrences inside [s, e) — what the children leave of it
                const long long s = (long long)(kh >> 8), e = (long long)lengths[i] - (long long)(kt >> 8);
                long long ranges = 0, bp = 0, from = s;
                if (a != b) {
                    for (uint64_t k = a; k < b; ++k) {
                        if (c_ranges[2 * k] > from) { ++ranges; bp += c_ranges[2 * k] - from; }
                        from = c_ranges[2 * k + 1];
                    }
                    if (from < e) { ++ranges; bp += e - from; }
                } else if (res.first[i] == -1 && s < e) {
                    ranges = 1; bp = e - s;
                }
                os << "          middle adapters = " << ranges << " ranges (" << bp << " bp)\n";
            }
        }
        if (run.endtrim_cuts)  // --trim_ends_q: the bases cut off either end, behind the lines of the parent's block
            os << "          quality trim = start " << run.endtrim_cuts[2 * i] << ", end " << run.endtrim_cuts[2 * i + 1] << "\n";
        if (run.screen_hits)  // --exclude: behind the lines of the parent's block
            os << "          excluded = " << (run.screen_excluded[i] ? "yes" : "no") << " (" << run.screen_hits[i] << " of "
               << (lengths[i] >= run.exclude_k ? lengths[i] - run.exclude_k + 1 : 0) << " " << run.exclude_k << "-mers)\n";
        if (run.complexity_bad)  // --max_low_complexity: behind the excluded line, if any
            os << "          low complexity = " << (run.complexity_flagged[i] ? "yes" : "no") << " (" << run.complexity_bad[i] << " of "
               << (lengths[i] >= 64 ? lengths[i] - 63 : 0) << " windows)\n";
        if (a != b) {
            for (uint64_t k = a; k < b; ++k) {
                os << "\n" << rname << "_" << c_ranges[2 * k] + 1 << "-" << c_ranges[2 * k + 1] << "\n";
                os << "            length = " << pad(std::to_string(c_ranges[2 * k + 1] - c_ranges[2 * k]), 11) << "mean quality = "
                          << double_to_string(c_mean[k]) << "      window quality = " << double_to_string(c_window[k]) << "\n";
            }
        }
    }
}

// rank 0: what the ranks behind it left in their files of this kind, in rank = file order
static bool print_verbose_parts(const Run &run, const char *kind) {
    std::vector<char> vbuf(1 << 20);
    for (int r = 1; r < run.world; ++r) {
        const std::string pth = run.part_path(kind, r);
        FILE *f = fopen(pth.c_str(), "rb");
        if (!f) { std::cerr << "Error: cannot read " << pth << "\n"; return false; }
        size_t got;
        while ((got = fread(vbuf.data(), 1, vbuf.size(), f)) > 0) std::cerr.write(vbuf.data(), (std::streamsize)got);
        fclose(f);
        unlink(pth.c_str());
    }
    return true;
}

// Read::print_verbose_read_info, src/read.cpp:169-194, in file order like the pass-1 loop (main.cpp:110-111).  Several ranks:
// rank r > 0 leaves the blocks of its reads in a file of the job's private directory; rank 0 prints its own and, behind the
// exchange of the totals (every rank has written its file when that returns), the others' in rank = file order.
static int print_verbose_blocks(const Run &run, const Pass1 &p, const flx_scores &res) {
    if (!run.args.verbose) return kGoOn;
    if (run.rank == 0) {
        print_read_blocks(std::cerr, run, p, res, p.lengths.size());
    } else {
        std::ofstream f(run.part_path("vblocks", run.rank), std::ios::binary);
        print_read_blocks(f, run, p, res, p.lengths.size());
        f.close();
        if (!f) return run.fail("verbose part");
    }
    if (run.world == 1) std::cerr << "\n";  // the line main.cpp:129 prints after the loop
    return kGoOn;
}

// src/main.cpp:199-214: the table shows the NORMALISED qualities and the final score, host libm like the reference
static int print_verbose_table(const Run &run, const Reads2 &r2, const flx_cut_report &rep) {
    const Args &args = run.args;
    const int rank = run.rank;
    if (!args.verbose) return kGoOn;
    std::ofstream table_file;
    if (rank > 0) table_file.open(run.part_path("vtable", rank), std::ios::binary);
    std::ostream &tos = rank > 0 ? (std::ostream &)table_file : (std::ostream &)std::cerr;
    if (rank == 0)
        std::cerr << "\n\n" << "Read name" << "\t" << "Length score" << "\t" << "Mean quality score" << "\t" << "Window quality score"
                  << "\t" << "Final score" << "\n";
    const double zspan = rep.max_z - rep.min_z;
    double (*volatile powfn)(double, double) = pow;
    for (uint64_t i = 0; i < r2.reads.size(); ++i) {
        double ratio = r2.window[i] / r2.mean[i];  // main.cpp:203-208
        if (ratio > 1.0) ratio = 1.0;
        const double z = (r2.mean[i] - rep.mean_quality) / rep.stdev_quality;
        const double mq = 100.0 * (z - rep.min_z) / zspan;
        const double wq = mq * ratio;
        const double lscore = 100.0 * (1.0 + (-5000.0 / (r2.len[i] + 5000.0)));
        // Read::set_final_score, read.cpp:249-267
        const double product = powfn(lscore, args.length_weight) * powfn(mq, args.mean_q_weight);
        const double gm = powfn(product, 1.0 / (args.length_weight + args.mean_q_weight));
        double scale = 1.0;
        if (mq > 0.0) scale = std::min(wq / mq, 1.0);
        const double wfrac = args.window_q_weight / (args.length_weight + args.mean_q_weight + args.window_q_weight);
        const double fs = gm * ((1.0 - wfrac) + (scale * wfrac));
        tos << pad(r2.reads[i].name, r2.longest_name) << "\t" << double_to_string(lscore) << "\t" << double_to_string(mq) << "\t"
            << double_to_string(wq) << "\t" << double_to_string(fs) << "\n";
    }
    if (run.world > 1) {  // every rank's rows are in its file when this exchange returns; rank 0 prints them in rank = file order
        if (rank > 0) { table_file.close(); if (!table_file) return run.fail("verbose part"); }
        uint64_t one = 1;
        if (flx_comm_sum_u64(run.ctx, &one, 1) != FLX_OK) return run.fail("exchange");
        if (rank == 0 && !print_verbose_parts(run, "vtable")) return 1;
    }
    if (rank == 0) std::cerr << "\n";
    return kGoOn;
}
