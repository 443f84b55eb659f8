// pass1.h — pass 1 over the long reads (src/main.cpp:63-130): open the input, check every record in file order, pack this rank's
// records chunk by chunk into the scoring pipeline.  One function per kind of input: mapped whole file, mapped rank range,
// streamed blocks.
#pragma once
#include <algorithm>
#include <climits>

#include "format.h"
#include "run.h"
#include "verbose.h"

// Two kinds of input.  A plain file is mapped and parsed in one piece (one batch): its record views stay valid, so the
// output pass needs no second parse, and every rank can index it.  A gzip file is STREAMED on one GPU: a block is
// inflated, its complete records are checked, packed and submitted, and the block's memory is reused; the output pass
// inflates the file a second time, like the reference's pass 2 (src/main.cpp:263-313).  Pipes cannot be read twice and
// several ranks need the record count before they score: both are inflated into memory.
struct ReadsInput {
    Input data;
    BlockReader blocks;
    bool streamed = false;
    uint64_t counted = UINT64_MAX;  // streamed input, several ranks: what rank 0's count pass saw
    uint64_t share_lo = 0, share_n = UINT64_MAX;  // streamed input, several ranks: this rank's records [share_lo, share_lo + share_n) of file order
    bool in_share(uint64_t rec) const { return rec >= share_lo && rec - share_lo < share_n; }
};

static int open_reads_input(Run &run, ReadsInput &in) {
    const Args &args = run.args;
    {
        const int fd = ::open(args.input_reads.c_str(), O_RDONLY);
        if (fd < 0) { std::cerr << "Error reading " << args.input_reads << "\n"; return 1; }
        unsigned char magic[2] = {0, 0};
        struct stat st;
        const bool regular = fstat(fd, &st) == 0 && S_ISREG(st.st_mode) && st.st_size > 0;
        const bool gz = regular && pread(fd, magic, 2, 0) == 2 && magic[0] == 0x1f && magic[1] == 0x8b;
        ::close(fd);
        // Several ranks (round 5): a gzip input is streamed by every rank as well — rank 0 counts the records in a pass of its own, the
        // count fixes every rank's contiguous share, then every rank streams the file, runs the checks of src/main.cpp:84-117 over
        // ALL records (they are per-record facts: every rank finds the same error at the same record) and packs and scores only its
        // share.  Up to round 4 every rank inflated the whole file into its memory.  (--verbose keeps that path: on an error it
        // scores the reads in front of it, all of them on rank 0.)
        // By default for compressed files of 1 GiB and more: below that the whole text fits every rank's memory easily and one pass is
        // quicker than two (measured with 8 ranks on 0.37 GB of gzip: 4.95 s streamed, 4.63 s in memory, and no smaller resident set —
        // the HIP runtime, the pinned slots and the inflater's buffers are 3.5 GB per rank either way; profiles/r05_gz_ranks.log).
        // FLX_CLI_RANK_STREAM=1: always (tests), =0: never.
        const char *rs_env = getenv("FLX_CLI_RANK_STREAM");
        const bool rank_stream = !args.verbose && (rs_env ? rs_env[0] != '0' : (gz && st.st_size >= ((off_t)1 << 30)));
        in.streamed = regular && (run.world == 1 || rank_stream) && !getenv("FLX_CLI_NO_STREAM") && (gz || getenv("FLX_CLI_FORCE_STREAM"));
        if (gz) {  // unaligned BAM (bam.h) is always taken into memory: Input::open turns it into FASTQ text, on every rank
            MappedFile file;
            if (file.open(args.input_reads) && bam_detect(file.p, file.n)) in.streamed = false;
        }
        in.data.bam = &kBamHooks;
        in.data.keep_bam = args.bam && !args.trim && !args.split_set && !args.split_window_q_set && !args.trim_adapters_set && !args.trim_ends_q_set;  // (--bam: the reads go out whole, as their original records)
    }
    if (in.streamed ? !in.blocks.open(args.input_reads, true) : !in.data.open(args.input_reads)) {
        if (!in.streamed && !in.data.bam_error.empty()) std::cerr << "Error: could not read BAM input " << args.input_reads << ": " << in.data.bam_error << "\n";
        else std::cerr << "Error reading " << args.input_reads << "\n";
        return 1;
    }
    run.stage("read input file");
    return kGoOn;
}

// streamed input, several ranks: rank 0 counts the records, the count fixes every rank's share
static int count_pass(Run &run, ReadsInput &in) {
    if (!in.streamed || run.world == 1) return kGoOn;
    uint64_t n_all[2] = {0, 0};  // records, and whether the count pass could not open the file (every rank must learn that: advisor, round 5)
    if (run.rank == 0) {  // (a damaged stream counts the records in front of the damage: every rank ends there in its own pass)
        BlockReader counter;
        Parsed b;
        if (counter.open(run.args.input_reads, false)) {
            while (counter.next(b)) {
                n_all[0] += b.recs.size();
                if (b.status <= -2) break;
            }
        } else {
            n_all[1] = 1;
        }
    }
    if (!run.ready()) return 1;
    if (flx_comm_sum_u64(run.ctx, n_all, 2) != FLX_OK) return run.fail("exchange");
    if (n_all[1]) { std::cerr << "Error reading " << run.args.input_reads << "\n"; return 1; }
    in.counted = n_all[0];
    const Share s = rank_share(n_all[0], run.world, run.rank);
    in.share_lo = s.lo;
    in.share_n = s.cnt;
    run.stage("count pass (rank 0)");
    return kGoOn;
}

// Packs records into the pipeline's pinned staging buffers (two slots: the GPU copies and scores chunk k while the host threads
// pack chunk k+1); only per-read scalars survive a chunk.
struct Scorer {
    Run &run;
    const bool streamed;
    flx_pipeline *pipe = nullptr;
    // two pinned staging slots of this size: pinning costs ~0.2 s per GiB and again when unpinned, so the slots are kept at
    // 256 MiB (profiles/r03_e2e.txt: 1 GiB slots cost a 2 GB input 0.45 s of 1.3 s)
    uint64_t chunk_bytes, chunk_reads = 4u << 20, n_chunks = 0;
    std::vector<uint64_t> offsets;

    Scorer(Run &r, bool streamed_input) : run(r), streamed(streamed_input) {
        chunk_bytes = streamed ? std::max<uint64_t>(4096, BlockReader::block_bytes()) : 256ull << 20;
        if (const char *e = getenv("FLX_CLI_CHUNK_MB")) chunk_bytes = std::max<uint64_t>(1, (uint64_t)atoll(e)) << 20;
        if (const char *e = getenv("FLX_CLI_CHUNK_BYTES")) chunk_bytes = std::max<uint64_t>(4096, (uint64_t)atoll(e));  // tests force many chunks
    }
    Scorer(const Scorer &) = delete;
    ~Scorer() { destroy(); }  // an error return must not leave the worker thread running into the runtime's teardown
    void destroy() { if (pipe) { flx_pipeline_destroy(pipe); pipe = nullptr; } }
    bool create_pipe() {  // if no record has come yet
        if (pipe) return true;
        if (flx_pipeline_create(run.ctx, run.kmers_empty ? nullptr : run.kmers, &run.prm, chunk_bytes, chunk_reads, &pipe) != FLX_OK) return false;
        // --split_window_q: the pipeline then splits the reads at their low-quality windows and returns children, as --split does
        if (run.args.split_window_q_set && flx_pipeline_set_qsplit(pipe, run.args.split_window_q) != FLX_OK) return false;
        // --exclude: the pipeline also screens every chunk against the contaminant's set; in Phred mode a chunk then carries the sequences
        // as a second plane behind the qualities
        if (run.excluding() && run.set_pipeline_screen(pipe) != FLX_OK) return false;
        // --trim_adapters: the pipeline cuts the adapters off the read ends and returns at most one child per read (with --split_adapters
        // the object also splits at the adapters inside a read: any number of children); the same second plane
        if (run.adapters && flx_pipeline_set_adapters(pipe, run.adapters) != FLX_OK) return false;
        // --trim_ends_q: the pipeline cuts the low-quality ends off the reads and returns at most one child per read; the qualities suffice
        if (run.args.trim_ends_q_set && flx_pipeline_set_endtrim(pipe, run.args.trim_ends_q) != FLX_OK) return false;
        // --max_low_complexity: the pipeline also counts the bad windows of every read, behind the screen; the same second plane
        return !run.low_complexity() ||
               flx_pipeline_set_complexity(pipe, run.args.max_low_complexity, (int)run.args.low_complexity_score) == FLX_OK;
    }

    // Pack records [lo, lo + cnt) of a batch chunk by chunk; their lengths are appended to `lengths`.
    int submit(std::vector<int32_t> &lengths, const std::vector<Record> &recs, uint64_t lo, uint64_t cnt) {
        if (!run.ready()) return 1;
        const uint64_t base = lengths.size();
        int32_t longest = 0;
        for (uint64_t i = 0; i < cnt; ++i) {
            if (recs[lo + i].seq.size() > (size_t)INT32_MAX) {  // the reference holds a read's length in an int as well (src/main.cpp:108)
                std::cerr << "\nError: read " << recs[lo + i].name.sv() << " is longer than 2^31-1 bases\n";
                return 1;
            }
            lengths.push_back((int32_t)recs[lo + i].seq.size());
            longest = std::max(longest, lengths.back());
        }
        const uint64_t need = (((uint64_t)longest + 15) & ~15ull) + 256;  // a read is never split over chunks
        if (!pipe) {
            if (!streamed) {  // everything is known: no larger slots than this rank's reads need
                uint64_t total = 4096;
                for (uint64_t i = 0; i < cnt; ++i) total += (((uint64_t)lengths[base + i] + 15) & ~15ull) + (lengths[base + i] >= 1024 ? 128 : 0);
                chunk_bytes = std::min(chunk_bytes, total);
                // small inputs: at least ~8 chunks, so that copy and scoring overlap the packing (but not below 64 MiB)
                if (!getenv("FLX_CLI_CHUNK_MB") && !getenv("FLX_CLI_CHUNK_BYTES"))
                    chunk_bytes = std::min(chunk_bytes, std::max<uint64_t>(total / 8, 64ull << 20));
                chunk_reads = std::min<uint64_t>(chunk_reads, std::max<uint64_t>(1, cnt));
            }
            chunk_bytes = std::max(chunk_bytes, need);
            if (!create_pipe()) return run.fail("pipeline");
        } else if (need > chunk_bytes) {
            chunk_bytes = need;
            if (flx_pipeline_reserve(pipe, chunk_bytes, chunk_reads) != FLX_OK) return run.fail("pipeline");
        }
        const int32_t *len = lengths.data() + base;
        const bool phred = run.kmers_empty;
        const bool second_plane = phred && (run.excluding() || run.adapters != nullptr || run.low_complexity());
        for (uint64_t at = 0; at < cnt;) {
            // the next chunk: as many records as fit the slot (flx_plane_layout's rule: 16-byte slots, 128-byte starts for long reads)
            uint64_t end = at, bytes = 0;
            while (end < cnt && end - at < chunk_reads) {
                uint64_t off = bytes;
                if (len[end] >= 1024) off = (off + 127u) & ~(uint64_t)127u;
                const uint64_t nb = off + (((uint64_t)len[end] + 15u) & ~(uint64_t)15u);
                if (nb > chunk_bytes && end > at) break;
                bytes = nb;
                ++end;
            }
            const uint64_t m = end - at;
            offsets.assign(m, 0);
            uint64_t plane_bytes = 0;
            flx_plane_layout(len + at, m, offsets.data(), &plane_bytes);
            uint8_t *plane = nullptr;
            if (flx_pipeline_next_buffer(pipe, &plane, nullptr, nullptr) != FLX_OK) return run.fail("scoring");
            const size_t parts = std::min<uint64_t>(m, (uint64_t)host_threads() * 8);
            parallel_for(parts, [&](size_t k) {  // byte-balanced slices of the chunk's reads
                const uint64_t lo_b = plane_bytes / parts * k, hi_b = k + 1 == parts ? plane_bytes : plane_bytes / parts * (k + 1);
                const uint64_t first = std::lower_bound(offsets.begin(), offsets.end(), lo_b) - offsets.begin();
                const uint64_t last = k + 1 == parts ? m : std::lower_bound(offsets.begin(), offsets.end(), hi_b) - offsets.begin();
                for (uint64_t i = first; i < last; ++i) {
                    const Record &r = recs[lo + at + i];
                    const View &src = phred ? r.qual : r.seq;  // Phred mode reads qual, k-mer mode reads seq
                    if (!src.empty()) memcpy(plane + offsets[i], src.p, src.size());
                    const uint64_t tail = offsets[i] + src.size();  // the staging buffer is reused: clear the padding behind the read
                    const uint64_t next = i + 1 < m ? offsets[i + 1] : plane_bytes;
                    if (next > tail) memset(plane + tail, 0, next - tail);
                    if (second_plane) {  // the sequences, at the same offsets behind the qualities
                        uint8_t *plane2 = plane + plane_bytes;
                        const size_t nseq = std::min<size_t>(r.seq.size(), (size_t)len[at + i]);
                        if (nseq) memcpy(plane2 + offsets[i], r.seq.p, nseq);
                        if (next > offsets[i] + nseq) memset(plane2 + offsets[i] + nseq, 0, next - (offsets[i] + nseq));
                    }
                }
            });
            if (flx_pipeline_submit(pipe, plane_bytes, offsets.data(), len + at, m) != FLX_OK) return run.fail("scoring");
            at = end;
            ++n_chunks;
        }
        return kGoOn;
    }
    // the scores of everything submitted, `n` reads (`report`: say why on stderr when that fails)
    int finish(flx_scores &res, uint64_t n, bool report = true) {
        if (!run.ready()) return 1;
        if (!create_pipe()) return report ? run.fail("pipeline") : 1;
        uint64_t n_scored = 0;
        if (flx_pipeline_finish(pipe, &res, &n_scored) != FLX_OK || n_scored != n) return report ? run.fail("scoring") : 1;
        if (run.excluding() && flx_pipeline_screen(pipe, &run.screen_hits, &run.screen_excluded) != FLX_OK) return report ? run.fail("scoring") : 1;
        if (run.adapters && flx_pipeline_adapters(pipe, &run.adapter_keys) != FLX_OK) return report ? run.fail("scoring") : 1;
        if (run.args.trim_ends_q_set && flx_pipeline_endtrim(pipe, &run.endtrim_cuts) != FLX_OK) return report ? run.fail("scoring") : 1;
        if (run.low_complexity() && flx_pipeline_complexity(pipe, &run.complexity_bad, &run.complexity_flagged) != FLX_OK) return report ? run.fail("scoring") : 1;
        return kGoOn;
    }
};

// --verbose on an ERROR path: the reference scores and prints every read inside its pass-1 loop, so the blocks of the reads in
// front of the failing record (for a duplicate name: that record's too) are on stderr before the error line
// (src/main.cpp:108-117).  Scoring is batched here: the reads read so far are scored now, then their blocks printed.
static void verbose_before_error(Run &run, Pass1 &p, Scorer &scorer, const std::vector<Record> &recs, uint64_t k) {
    if (!run.args.verbose || run.rank > 0) return;  // (several ranks: rank 0 alone scores the reads in front of the error — no exchange is involved)
    if (!scorer.streamed) for (uint64_t i = 0; i < k; ++i) p.names.push_back(recs[i].name.sv());
    if (scorer.submit(p.lengths, recs, 0, k) != kGoOn) return;
    flx_scores res;
    if (scorer.finish(res, p.lengths.size(), false) != kGoOn) return;
    print_read_blocks(std::cerr, run, p, res, p.lengths.size());
}

// An error of the INPUT is found by every rank at the same record (all of them index the whole file): rank 0 reports it and
// ends the job; the others leave quietly with status 0, so that the watchdog does not take their exit for a rank that died
// while rank 0 is still scoring and printing the --verbose blocks in front of the error.
static int input_error_rc(const Run &run) { return run.rank > 0 ? 0 : 1; }

static uint64_t name_hash64(const View &v) {  // FNV-1a
    uint64_t h = 1469598103934665603ull;
    for (size_t q = 0; q < v.n; ++q) { h ^= (unsigned char)v.p[q]; h *= 1099511628211ull; }
    return h ^ (h >> 29);
}

// the progress line of src/main.cpp:119-127
static void print_progress(uint64_t n_reads, long long bases) {
    std::cerr << "\r  " << int_to_string((long long)n_reads) << " reads (" << int_to_string(bases) << " bp)";
}
// ... which comes whenever 483 611 more bases have been read; `n_reads` and `bases` include the read just taken
static void progress_step(uint64_t n_reads, long long bases, long long &last_progress, bool print) {
    if (bases - last_progress < 483611) return;
    last_progress = bases;
    if (print) print_progress(n_reads, bases);
}

// The per-record checks of src/main.cpp:84-117 for record k of a batch, in file order.  `duplicate`: an earlier record has this
// name.  `keep_name`: not null when the names are kept record by record (a streamed input, a record of this rank's share).
static int check_record(Run &run, Pass1 &p, Scorer &scorer, const std::vector<Record> &recs, uint64_t k, bool duplicate,
                        const std::string_view *keep_name) {
    const Record &r = recs[k];
    p.total_bases += (long long)r.seq.size();
    const bool fasta_format = r.qual.empty() && !r.seq.empty();
    const bool fastq_format = !r.qual.empty() && !r.seq.empty() && r.qual.size() == r.seq.size();
    p.any_fasta = p.any_fasta || fasta_format;
    p.any_fastq = p.any_fastq || fastq_format;
    if (p.any_fasta && p.any_fastq) {
        verbose_before_error(run, p, scorer, recs, k);
        std::cerr << "\n\n" << "Error: could not parse input reads" << "\n";
        std::cerr << "  problem occurred at read " << r.name << "\n";
        return input_error_rc(run);
    }
    if (fasta_format && run.kmers_empty) {
        verbose_before_error(run, p, scorer, recs, k);
        std::cerr << "\n\n" << "Error: FASTA input not supported without an external reference" << "\n";
        return input_error_rc(run);
    }
    if (keep_name) p.names.push_back(*keep_name);  // (a duplicate itself is scored and printed before the check, main.cpp:108-113)
    if (duplicate) {
        verbose_before_error(run, p, scorer, recs, k + 1);
        std::cerr << "Error: duplicate read name: " << r.name << "\n";
        return input_error_rc(run);
    }
    p.header_only.note(r, p.n_records);
    ++p.n_records;
    progress_step(p.n_records, p.total_bases, p.last_progress, !run.args.verbose);
    return kGoOn;
}

// the parser's own end status of a batch, behind the checks of its records
static int check_batch_end(Run &run, Pass1 &p, Scorer &scorer, const Parsed &batch) {
    if (batch.status == -2) {
        verbose_before_error(run, p, scorer, batch.recs, batch.recs.size());
        std::cerr << "Error: incorrect FASTQ format for read " << batch.bad.name << "\n";
        return input_error_rc(run);
    }
    if (batch.status == -3) {  // a damaged gzip stream: kseq's error state behind the bytes gzread delivered (src/main.cpp:85-88)
        verbose_before_error(run, p, scorer, batch.recs, batch.recs.size());
        std::cerr << "Error reading " << run.args.input_reads << "\n";
        return input_error_rc(run);
    }
    return kGoOn;
}

// Duplicate names in a mapped input (src/main.cpp:113-117: the first record whose name an earlier record has), or UINT64_MAX.
// Every thread owns the names whose hash falls into its share, walks the records in file order and stops at the first name it
// has seen before; the smallest such record over all threads is the reference's.
static uint64_t first_duplicate_name(const std::vector<Record> &recs) {
    uint64_t dup_at = UINT64_MAX;
    const size_t nrec = recs.size();
    if (nrec < 2) return dup_at;
    std::vector<uint64_t> name_hash(nrec);
    const size_t hparts = std::min<size_t>(nrec, 64);
    parallel_for(hparts, [&](size_t k) {
        for (size_t i = nrec * k / hparts; i < nrec * (k + 1) / hparts; ++i) name_hash[i] = name_hash64(recs[i].name);
    });
    const size_t owners = std::max<size_t>(1, std::min<size_t>(host_threads(), nrec / 4096));
    std::vector<uint64_t> first_dup(owners, UINT64_MAX);
    parallel_for(owners, [&](size_t t) {
        std::unordered_set<std::string_view> mine;
        mine.reserve(nrec / owners * 2 + 16);
        for (size_t i = 0; i < nrec; ++i)
            if (name_hash[i] % owners == t && !mine.insert(recs[i].name.sv()).second) { first_dup[t] = i; return; }
    });
    for (uint64_t d : first_dup) dup_at = std::min(dup_at, d);
    return dup_at;
}

// A mapped / in-memory input, every record: parse, duplicate search, checks, then this rank's contiguous block of file order by count.
static int pass1_mapped(Run &run, ReadsInput &in, Pass1 &p, Scorer &scorer) {
    p.kept = Parsed();
    parse_all(in.data, p.kept);
    run.stage("parse");
    const std::vector<Record> &recs = p.kept.recs;
    const uint64_t dup_at = first_duplicate_name(recs);
    for (uint64_t k = 0; k < recs.size(); ++k)
        if (const int rc = check_record(run, p, scorer, recs, k, k == dup_at, nullptr); rc != kGoOn) return rc;
    if (const int rc = check_batch_end(run, p, scorer, p.kept); rc != kGoOn) return rc;
    run.stage("record checks");
    const Share mine = rank_share(recs.size(), run.world, run.rank);
    p.lo_rec = mine.lo;
    p.names.reserve(mine.cnt);
    for (uint64_t i = 0; i < mine.cnt; ++i) p.names.push_back(recs[mine.lo + i].name.sv());
    return scorer.submit(p.lengths, recs, mine.lo, mine.cnt);
}

// two equal values among w[0, n)?  1024 buckets by the top bits, sorted concurrently
static bool any_value_twice(const std::vector<uint64_t> &w, uint64_t n) {
    const size_t NB = 1024;
    std::vector<size_t> at(NB + 1, 0);
    for (uint64_t i = 0; i < n; ++i) ++at[(w[i] >> 54) + 1];
    for (size_t b = 0; b < NB; ++b) at[b + 1] += at[b];
    std::vector<uint64_t> sorted(n);
    {
        std::vector<size_t> cur(at.begin(), at.end() - 1);
        for (uint64_t i = 0; i < n; ++i) sorted[cur[w[i] >> 54]++] = w[i];
    }
    std::vector<char> twice(NB, 0);
    parallel_for(NB, [&](size_t b) {
        std::sort(sorted.begin() + (ptrdiff_t)at[b], sorted.begin() + (ptrdiff_t)at[b + 1]);
        for (size_t i = at[b] + 1; i < at[b + 1]; ++i)
            if (sorted[i] == sorted[i - 1]) { twice[b] = 1; break; }
    });
    return std::find(twice.begin(), twice.end(), 1) != twice.end();
}

// ---- several ranks, a mapped file: every rank indexes only ITS byte range (round-3 review, item 8a; the default since round 5,
// after the ranks fuzz, the damaged-input fuzz and the CLI's multi-rank tests had been through it; FLX_CLI_RANK_RANGES=0 switches it off).  parse_rank_range gives the share; what pass1_mapped checks record by record
// over the whole file becomes three facts about the shares and two exchanges:
//   * every share is accepted and made of ordinary records of ONE kind (FASTQ with as many qualities as bases, or FASTA in k-mer
//     mode), none empty, none longer than an int: a sum of flags.  Anything else — an error to report in file order, records
//     whose output depends on the ones in front of them (the header-only records of run.h) — and EVERY rank parses the whole file
//     as before: the odd cases keep the code that is checked against the reference, and they are cheap or fatal anyway;
//   * no name occurs twice: the 64-bit hashes of all names, gathered (a sum into disjoint slots) and sorted on every rank; two
//     equal hashes — a duplicate or a collision — send every rank to the whole file as well;
//   * the progress lines of src/main.cpp:119-127 depend on every read's length in file order: gathered with the hashes, rank 0
//     replays them.
// 0: not taken (parse the whole file), 1: `mine` holds this rank's records and the totals are set, -1: the exchange failed.
static int index_rank_range(Run &run, const ReadsInput &in, Pass1 &p, Parsed &mine) {
    const int rank = run.rank, world = run.world;
    bool ok = parse_rank_range(in.data, rank, world, mine);
    bool fa = false, fq = false;
    uint64_t bases = 0;
    if (ok)
        for (const Record &r : mine.recs) {
            const bool fasta_format = r.qual.empty() && !r.seq.empty() && !r.is_fastq;
            const bool fastq_format = r.is_fastq && !r.seq.empty() && r.qual.size() == r.seq.size();
            if ((!fasta_format && !fastq_format) || r.seq.size() > (size_t)INT32_MAX) { ok = false; break; }
            fa = fa || fasta_format;
            fq = fq || fastq_format;
            bases += r.seq.size();
        }
    const uint64_t n_mine = ok ? mine.recs.size() : 0;
    std::vector<uint64_t> v(3 + 2 * (size_t)world, 0);
    v[0] = ok; v[1] = ok && fa; v[2] = ok && fq;
    v[3 + (size_t)rank] = n_mine;
    v[3 + (size_t)world + (size_t)rank] = ok ? bases : 0;
    if (flx_comm_sum_u64(run.ctx, v.data(), v.size()) != FLX_OK) return -1;
    if (v[0] != (uint64_t)world || (v[1] && v[2]) || (v[1] && run.kmers_empty)) return 0;
    uint64_t n_all = 0, lo = 0, bases_all = 0;
    for (int r = 0; r < world; ++r) {
        if (r == rank) lo = n_all;
        n_all += v[3 + (size_t)r];
        bases_all += v[3 + (size_t)world + (size_t)r];
    }
    // names and lengths of every read, in file order: hashes in [0, n_all), lengths two to a word behind them
    std::vector<uint64_t> w(n_all + (n_all + 1) / 2, 0);
    const size_t parts = std::min<size_t>(std::max<size_t>(1, n_mine), 64);
    parallel_for(parts, [&](size_t k) {
        for (size_t i = n_mine * k / parts; i < n_mine * (k + 1) / parts; ++i) w[lo + i] = name_hash64(mine.recs[i].name);
    });
    for (uint64_t i = 0; i < n_mine; ++i)  // (serial: two neighbours share a word)
        w[n_all + ((lo + i) >> 1)] |= (uint64_t)(uint32_t)mine.recs[i].seq.size() << (32 * ((lo + i) & 1));
    if (flx_comm_sum_u64(run.ctx, w.data(), w.size()) != FLX_OK) return -1;
    if (any_value_twice(w, n_all)) return 0;
    p.n_records = n_all;
    p.total_bases = (long long)bases_all;
    p.any_fasta = v[1] != 0;
    p.any_fastq = v[2] != 0;
    if (rank == 0 && !run.args.verbose) {  // the progress lines, as check_record prints them read by read
        long long tb = 0, lp = 0;
        for (uint64_t i = 0; i < n_all; ++i) {
            tb += (long long)((w[n_all + (i >> 1)] >> (32 * (i & 1))) & 0xffffffffull);
            progress_step(i + 1, tb, lp, true);
        }
    }
    return 1;
}

// A mapped file, several ranks: this rank's byte range alone, when index_rank_range takes it (`taken`); else pass1_mapped follows.
static int pass1_rank_range(Run &run, ReadsInput &in, Pass1 &p, Scorer &scorer, bool &taken) {
    const char *rr_env = getenv("FLX_CLI_RANK_RANGES");  // "0": every rank parses the whole file (round 4's default; tests, A/B)
    taken = false;
    if (run.world == 1 || in.data.map == nullptr || (rr_env && rr_env[0] == '0')) return kGoOn;
    const int took = index_rank_range(run, in, p, p.kept);
    if (took < 0) return run.fail("exchange");
    if (took == 0) return kGoOn;
    taken = true;
    run.stage("parse");
    // every check of check_record has been made for the whole file (index_rank_range): this rank's records are its share
    const std::vector<Record> &recs = p.kept.recs;
    p.lo_rec = 0;
    p.names.reserve(recs.size());
    for (const Record &r : recs) p.names.push_back(r.name.sv());
    if (run.timing) fprintf(stderr, "[timing] rank ranges: %llu of %llu records indexed here\n", (unsigned long long)recs.size(), (unsigned long long)p.n_records);
    return scorer.submit(p.lengths, recs, 0, recs.size());
}

// A streamed input, block after block: the checks over ALL records, packing and scoring of this rank's share.
static int pass1_streamed(Run &run, ReadsInput &in, Pass1 &p, Scorer &scorer) {
    BlockReader &blocks = in.blocks;
    std::unordered_set<std::string_view> seen_names;
    Parsed batch;
    p.lo_rec = in.share_lo;
    while (blocks.next(batch)) {
        const std::vector<Record> &recs = batch.recs;
        for (uint64_t k = 0; k < recs.size(); ++k) {
            p.name_arena.emplace_back(recs[k].name.sv());  // the block's memory is reused: keep a copy
            const std::string_view name = p.name_arena.back();
            const bool duplicate = !seen_names.insert(name).second;
            const uint64_t index = p.n_records;
            if (const int rc = check_record(run, p, scorer, recs, k, duplicate, in.in_share(index) ? &name : nullptr); rc != kGoOn) return rc;
            p.units.note_record(blocks.points, blocks.offset_of(recs[k].name.p - 1), index);
        }
        p.header_only.end_of_block();
        if (const int rc = check_batch_end(run, p, scorer, batch); rc != kGoOn) return rc;
        // the part of this block that lies in the rank's share (n_records has moved behind the block); one rank: everything
        const uint64_t first = p.n_records - recs.size(), last = p.n_records;
        const uint64_t a0 = std::max(first, in.share_lo), a1 = in.share_n == UINT64_MAX ? last : std::min(last, in.share_lo + in.share_n);
        if (const int rc = scorer.submit(p.lengths, recs, a0 < a1 ? a0 - first : 0, a0 < a1 ? a1 - a0 : 0); rc != kGoOn) return rc;
    }
    if (blocks.io_error) { std::cerr << "Error reading " << run.args.input_reads << "\n"; return input_error_rc(run); }
    p.units.finish(blocks.points, blocks.end_offset(), p.n_records);
    if (in.counted != UINT64_MAX && p.n_records != in.counted) {
        // the shares were cut from rank 0's count: a file that changed between the two passes would give shares that do not match the records seen
        std::cerr << "Error: " << run.args.input_reads << " changed while it was read (" << in.counted << " records counted, " << p.n_records << " read)\n";
        return 1;
    }
    return kGoOn;
}
