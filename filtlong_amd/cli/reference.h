// reference.h — the reference files of -a / -1 / -2 as a STREAM into the device-side 16-mer set (src/kmers.cpp:75-134).
//
// The reference reads a record at a time through kseq and hashes it on the spot: constant memory, and a progress line
// "\r  file (N bp)" whenever 483 611 more bases have been hashed (src/kmers.cpp:123-126), once more at the end, then "\n".
// Here: a regular file — plain or gzip — goes through the block-wise reader (gzblocks.h: a block is inflated, the records that
// are complete inside it are parsed, the unfinished tail moves on), the sequences of at least 16 bases are packed back to back
// and handed to flx_kmerset_add_assembly / flx_kmerset_add_short_reads in batches of at most FLX_CLI_REF_BATCH_BYTES (256 MiB);
// the C ABI takes any number of such calls, in file order (include/filtlong_hip.h).  Host memory is O(block + batch) whatever the
// size of the file (round 4 held three copies of every sequence).  The progress lines are printed record by record with the
// reference's rule, so stderr is the reference's byte for byte.  Pipes and empty files keep the in-memory reader (fastx.h: Input).
#pragma once
#include <sys/stat.h>

#include "format.h"
#include "run.h"

static void print_hash_progress(const std::string &filename, long long base_count) {  // src/kmers.cpp (print_hash_progress)
    std::cerr << "\r  " << filename << " (" << int_to_string(base_count) << " bp)";
}

// every record of a reference file, in file order: a regular file — plain or gzip — block by block, a pipe or an empty file through
// the in-memory reader (FLX_CLI_NO_STREAM: always that one).  Any error ends the loop silently, like `while ((l = kseq_read(seq)) >= 0)`;
// so does keep_going() answering false.
template <class Take, class KeepGoing>
static void for_each_record(const std::string &filename, Take take, KeepGoing keep_going) {
    BlockReader blocks;
    if (!getenv("FLX_CLI_NO_STREAM") && blocks.open(filename, false)) {
        Parsed batch;
        while (keep_going() && blocks.next(batch)) {
            for (const Record &r : batch.recs) take(r);
            if (batch.status <= -2) break;
        }
    } else {
        Input data;
        std::deque<std::string> arena;
        if (data.open(filename)) {
            Parser p(data, arena);
            Record r;
            while (keep_going() && p.next(r) >= 0) {
                take(r);
                arena.clear();  // (the record's multi-line fields have been copied)
            }
        }
    }
}

// hashes one reference file: its sequences of at least 16 bases go to add(bases, offsets, lengths, n) in batches; returns the number
// of sequences (those shorter than 16 bases count too, src/kmers.cpp:96-100).  rc: what add answered last — not FLX_OK: the library
// refused a batch (flx_last_error says why) and the rest of the file was not read
template <class Add>
static int hash_reference(const std::string &filename, Add add, int &rc) {
    int n = 0;
    long long bases = 0, last_progress = 0;
    size_t batch_bytes = (size_t)256 << 20;
    if (const char *e = getenv("FLX_CLI_REF_BATCH_BYTES")) batch_bytes = std::max<size_t>(16, (size_t)atoll(e));  // tests force many batches
    std::vector<uint8_t> pack;
    std::vector<uint64_t> offsets;
    std::vector<int64_t> lengths;
    rc = FLX_OK;
    auto flush = [&]() {
        if (offsets.empty() || rc != FLX_OK) return;
        rc = add(pack.data(), offsets.data(), lengths.data(), (uint64_t)offsets.size());
        pack.clear();
        offsets.clear();
        lengths.clear();
    };
    auto take = [&](const Record &r) {  // one pass of the loop of src/kmers.cpp:91-127
        ++n;
        if (r.seq.size() < 16) return;
        bases += (long long)r.seq.size();
        if (pack.size() + r.seq.size() > batch_bytes) flush();
        offsets.push_back(pack.size());
        lengths.push_back((int64_t)r.seq.size());
        pack.insert(pack.end(), (const uint8_t *)r.seq.p, (const uint8_t *)r.seq.p + r.seq.size());
        if (bases - last_progress >= 483611) {
            last_progress = bases;
            print_hash_progress(filename, bases);
        }
    };
    for_each_record(filename, take, [&] { return rc == FLX_OK; });
    flush();
    print_hash_progress(filename, bases);
    std::cerr << "\n";
    return n;
}

// ---- reference 16-mers (src/main.cpp:51-59, src/kmers.cpp:50-72) --------------------------------------
static int build_reference_set(Run &run) {
    const Args &args = run.args;
    if (!args.assembly_set && args.short_reads.empty()) return kGoOn;
    if (flx_kmerset_create(run.ctx, &run.kmers) != FLX_OK) return run.fail("k-mer set");
    if (args.assembly_set) {
        std::cerr << "Hashing 16-mers from assembly\n";
        std::cerr << "  " << args.assembly << "\n";
        // the reference prints the set's size after the assembly alone (src/kmers.cpp:60-72); with short reads to follow that
        // takes a second set, which is fed the same batches and dropped once it has been counted
        flx_kmerset *alone = nullptr;
        if (!args.short_reads.empty() && flx_kmerset_create(run.ctx, &alone) != FLX_OK) return run.fail("k-mer set");
        int rc;
        const int count = hash_reference(args.assembly, [&](const uint8_t *bases, const uint64_t *offsets, const int64_t *lengths, uint64_t n) {
            const int first = flx_kmerset_add_assembly(run.kmers, bases, offsets, lengths, n);
            return first != FLX_OK || !alone ? first : flx_kmerset_add_assembly(alone, bases, offsets, lengths, n);
        }, rc);
        if (rc != FLX_OK) return run.fail("assembly");
        flx_kmerset *counted = alone ? alone : run.kmers;
        if (flx_kmerset_finalize(counted) != FLX_OK) return run.fail(alone ? "assembly" : "k-mer set");
        std::cerr << "  " << int_to_string(count) << " " << (count == 1 ? "contig" : "contigs") << ", "
                  << int_to_string((long long)flx_kmerset_size(counted)) << " 16-mers\n\n";
        if (alone) flx_kmerset_destroy(alone);
    }
    if (!args.short_reads.empty()) {
        std::cerr << "Hashing 16-mers from short reads\n";
        int count = 0;
        for (auto &f : args.short_reads) {
            int rc;
            count += hash_reference(f, [&](const uint8_t *bases, const uint64_t *offsets, const int64_t *lengths, uint64_t n) {
                return flx_kmerset_add_short_reads(run.kmers, bases, offsets, lengths, n);
            }, rc);
            if (rc != FLX_OK) return run.fail("short reads");
        }
        if (flx_kmerset_finalize(run.kmers) != FLX_OK) return run.fail("k-mer set");
        std::cerr << "  " << int_to_string(count) << " reads, " << int_to_string((long long)flx_kmerset_size(run.kmers)) << " 16-mers\n\n";
    }
    run.kmers_empty = flx_kmerset_size(run.kmers) == 0;
    return kGoOn;
}

// ---- --exclude FILE: the contaminant's 16-mers, a set of its own beside the reference's.  Every rank builds it itself, through the
// reader of -a (gzip included, in batches); flx_screen_set_add cuts the sequences at every byte outside ACGTacgt.  16-mers cannot
// screen a large genome: an unrelated read keeps N / 2^32 of its windows, and once that background reaches half the threshold —
// N * 200 >= P * 2^32 — the run is refused.
// --exclude_k K, 17 <= K <= 31: the contaminant's canonical K-mers in a hash table on the device (csrc/screen_hash.h), which is what
// lets a genome be screened.  The table starts at twice the file's bytes, so that a plain FASTA is never rehashed (a gzip file grows
// as it is read).  The background of an unrelated read is at most 2 M / 4^K of its windows for M canonical keys; the rule above
// becomes M * 400 >= P * 4^K.
static int build_exclude_set(Run &run) {
    const Args &args = run.args;
    if (!args.exclude_set) return kGoOn;
    if (!run.ready()) return 1;
    // what the two kinds of set differ in: K, the calls, the noun of the count line, the background rule (refused when
    // n * factor >= P * space) and, for the hashed kind, a message of its own for FLX_ERR_NOMEM from create or add
    const bool hashed = args.exclude_k > 16;
    const int k = hashed ? (int)args.exclude_k : 16;
    const long double factor = hashed ? 400.0L : 200.0L, space = hashed ? (long double)(1ull << (2 * k)) : 4294967296.0L;
    const char *no_memory = "Error: not enough device memory for the --exclude set\n";
    int rc;
    if (hashed) {
        struct stat st;
        const uint64_t file_bytes = stat(args.exclude.c_str(), &st) == 0 && st.st_size > 0 ? (uint64_t)st.st_size : 0;
        int hint = 16;
        while (hint < 40 && (1ull << hint) < 2 * file_bytes) ++hint;
        rc = flx_screenset_create(run.ctx, k, hint, &run.exclude_hash);
    } else {
        rc = flx_kmerset_create(run.ctx, &run.exclude);
    }
    if (hashed && rc == FLX_ERR_NOMEM) { std::cerr << no_memory; return 1; }
    if (rc != FLX_OK) return run.fail("exclude set");
    run.exclude_k = k;
    std::cerr << "Hashing " << k << "-mers to exclude\n";
    std::cerr << "  " << args.exclude << "\n";
    const int count = hash_reference(args.exclude, [&](const uint8_t *bases, const uint64_t *offsets, const int64_t *lengths, uint64_t n) {
        return hashed ? flx_screenset_add(run.exclude_hash, bases, offsets, lengths, n) : flx_screen_set_add(run.exclude, bases, offsets, lengths, n);
    }, rc);
    if (hashed && rc == FLX_ERR_NOMEM) { std::cerr << no_memory; return 1; }
    if (rc != FLX_OK) return run.fail("exclude");
    if ((hashed ? flx_screenset_finalize(run.exclude_hash) : flx_kmerset_finalize(run.exclude)) != FLX_OK) return run.fail("exclude set");
    const uint64_t n = hashed ? flx_screenset_size(run.exclude_hash) : flx_kmerset_size(run.exclude);
    std::cerr << "  " << int_to_string(count) << " " << (count == 1 ? "sequence" : "sequences") << ", " << int_to_string((long long)n) << " " << (hashed ? "canonical " : "") << k
              << "-mers\n\n";
    if ((long double)n * factor >= (long double)args.exclude_percent * space) {
        std::cerr << "Error: the reference for --exclude holds too many " << k << "-mers (" << n << ") for --exclude_percent " << args.exclude_percent_text << "\n";
        return 1;
    }
    if (n == 0) { std::cerr << "Error: the reference for --exclude holds no " << k << "-mer of ACGT\n"; return 1; }
    return kGoOn;
}

// ---- --trim_adapters FILE: the adapters' sequences, through the reader of -a (gzip included).  Every rank reads the file itself; the
// patterns belong to no device until the first chunk asks for them.
static int build_adapters(Run &run) {
    const Args &args = run.args;
    if (!args.trim_adapters_set) return kGoOn;
    std::cerr << "Reading adapters\n";
    std::cerr << "  " << args.trim_adapters << "\n";
    std::vector<uint8_t> pack;
    std::vector<uint64_t> offsets;
    std::vector<int64_t> lengths;
    auto take = [&](const Record &r) {
        run.adapter_names.push_back(std::string(r.name.sv()));
        offsets.push_back(pack.size());
        lengths.push_back((int64_t)r.seq.size());
        pack.insert(pack.end(), (const uint8_t *)r.seq.p, (const uint8_t *)r.seq.p + r.seq.size());
    };
    for_each_record(args.trim_adapters, take, [] { return true; });
    const size_t count = offsets.size();
    std::cerr << "  " << int_to_string((long long)count) << " " << (count == 1 ? "sequence" : "sequences") << "\n";
    if (args.adapter_overhang > 0) std::cerr << "  overhang: up to " << args.adapter_overhang << " bases\n";  // --adapter_overhang (0 prints nothing)
    std::cerr << "\n";
    for (size_t i = 0; i < count; ++i) {
        bool good = lengths[i] >= 12 && lengths[i] <= 64;
        for (int64_t k = 0; good && k < lengths[i]; ++k) good = strchr("ACGTacgt", (char)pack[offsets[i] + (uint64_t)k]) != nullptr && pack[offsets[i] + (uint64_t)k] != 0;
        if (!good) { std::cerr << "Error: adapter " << run.adapter_names[i] << " must have 12 to 64 bases of ACGT\n"; return 1; }
    }
    if (count == 0) { std::cerr << "Error: the file for --trim_adapters holds no sequence\n"; return 1; }
    if (count > 128) { std::cerr << "Error: the file for --trim_adapters holds more than 128 sequences\n"; return 1; }
    if (flx_adapters_create(pack.data(), offsets.data(), lengths.data(), count, (int)args.adapter_errors, (int)args.adapter_window, &run.adapters) != FLX_OK) {
        std::cerr << "Error: the adapters of " << args.trim_adapters << " were refused\n";
        return 1;
    }
    // --split_adapters: the same patterns are also searched inside the reads
    if (args.split_adapters && flx_adapters_set_split(run.adapters, (int)args.adapter_split_errors) != FLX_OK) {
        std::cerr << "Error: the adapters of " << args.trim_adapters << " were refused\n";
        return 1;
    }
    // --adapter_overhang: adapters that a read begins or ends inside are found as well
    if (args.adapter_overhang > 0 && flx_adapters_set_overhang(run.adapters, (int)args.adapter_overhang) != FLX_OK) {
        std::cerr << "Error: the adapters of " << args.trim_adapters << " were refused\n";
        return 1;
    }
    return kGoOn;
}
