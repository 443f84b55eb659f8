// output.h — the output pass (src/main.cpp:263-313 writes record by record).  Its engine: n independent pieces produced by several
// threads, written in order or, into a regular file, each at its own offset.  Around it: how a read of reads2 is cut out of its
// record, the pass over a mapped input, the pass over a streamed one, and what the ranks do to end up with ONE output.
#pragma once
#include <atomic>
#include <condition_variable>
#include <mutex>
#include <thread>
#include <vector>

#include <fcntl.h>
#include <sys/stat.h>
#include <sys/uio.h>
#include <unistd.h>

#include "pass1.h"
#include "run.h"

// ---- ordered pieces ----------------------------------------------------------------------------------------------------
// The output is produced as `n` independent pieces by several threads.  produce(j, piece, target) fills piece j and says whether it
// could.  With `offsets` (n + 1 byte offsets, the sink a regular file that is not in append mode) every thread writes its
// own pieces with pwrite at base + offsets[j] and the file position is moved behind the last one; without, this thread
// writes the pieces in order as they become ready, and no more than 2 x threads of them exist at a time.
// produce(j, piece, target) is told where the pieces go: `direct`, the producers may write their pieces themselves (pwrite to `fd` at
// `base` + the piece's offset, leaving `piece` empty).
struct PieceTarget { bool direct; int fd; off_t base; };
static int g_shared_out = -1;         // ranks forked by --gpus N: a duplicate of the job's stdout (the SAME open file in every rank)
// `forced_base` >= 0: the sink is a regular file shared with other processes and this process's pieces start at that offset (the
// file position is then nobody's to move here)
template <class Produce>
static bool write_pieces(size_t n, Produce &&produce, FILE *sink, const std::vector<uint64_t> *offsets, off_t forced_base = -1) {
    fflush(sink);
    const int fd = fileno(sink);
    struct stat st;
    const int fl = fcntl(fd, F_GETFL);
    const off_t base = forced_base >= 0 ? forced_base : lseek(fd, 0, SEEK_CUR);
    const bool direct = offsets && (forced_base >= 0 || !getenv("FLX_CLI_ORDERED_OUTPUT")) && fstat(fd, &st) == 0 && S_ISREG(st.st_mode) && fl >= 0 &&
                        !(fl & O_APPEND) && base >= 0;
    if (forced_base >= 0 && !direct) return false;
    const PieceTarget target{direct, fd, base};
    std::vector<std::string> piece(n);
    std::vector<char> state(n, 0);  // 1: ready (or written), 2: failed
    std::mutex mu;
    std::condition_variable cv;
    std::atomic<size_t> next{0};
    size_t written = 0;
    const unsigned n_workers = (unsigned)std::max<size_t>(1, std::min<size_t>(host_threads(), n));
    const size_t ahead = 2 * (size_t)n_workers;
    auto worker = [&] {
        for (;;) {
            const size_t j = next.fetch_add(1);
            if (j >= n) return;
            if (!direct) {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return j < written + ahead; });
            }
            std::string &buf = piece[j];
            if (offsets && !direct) buf.reserve((size_t)((*offsets)[j + 1] - (*offsets)[j]));
            bool ok = produce(j, buf, target);
            const bool self_written = direct && ok && buf.empty() && (*offsets)[j + 1] != (*offsets)[j];  // the producer used pwritev itself
            if (offsets && !self_written) ok = ok && buf.size() == (*offsets)[j + 1] - (*offsets)[j];
            if (direct) {
                for (size_t done = 0; ok && done < buf.size();) {
                    const ssize_t w = pwrite(fd, buf.data() + done, buf.size() - done, base + (off_t)((*offsets)[j] + done));
                    if (w <= 0) ok = false;
                    else done += (size_t)w;
                }
                std::string().swap(buf);
            }
            {
                std::unique_lock<std::mutex> lk(mu);
                state[j] = ok ? 1 : 2;
            }
            cv.notify_all();
        }
    };
    std::vector<std::thread> pool;
    for (unsigned t = 0; t < n_workers; ++t) pool.emplace_back(worker);
    bool failed = false;
    for (size_t j = 0; j < n; ++j) {
        {
            std::unique_lock<std::mutex> lk(mu);
            cv.wait(lk, [&] { return state[j] != 0; });
            failed = failed || state[j] == 2;
        }
        if (!direct) {
            if (!failed && fwrite(piece[j].data(), 1, piece[j].size(), sink) != piece[j].size()) failed = true;  // (the producers run dry below)
            std::string().swap(piece[j]);
            {
                std::unique_lock<std::mutex> lk(mu);
                written = j + 1;
            }
            cv.notify_all();
        }
    }
    for (auto &t : pool) t.join();
    if (direct && forced_base < 0 && !failed && lseek(fd, base + (off_t)(*offsets)[n], SEEK_SET) < 0) failed = true;
    return !failed;
}

static int write_error() {
    std::cerr << "Error: could not write the output\n";
    return 1;
}

// --gzip: every piece is compressed into BGZF members by the worker that produced it (flx_bgzf may be called from all of them at
// once: ~16 MiB pieces are ~257 members each, so the concurrent workers are what keeps the device full); the pieces then go out
// in order like plain ones, and the end-of-file block follows once the output pass is complete.
static bool gz_piece(flx_bgzf *gz, std::string &buf) {
    if (!gz || buf.empty()) return true;
    uint64_t bound = 0, got = 0;
    if (flx_bgzf_bound(buf.size(), 0, &bound) != FLX_OK) return false;
    std::string z(bound, '\0');
    if (flx_bgzf_compress(gz, buf.data(), buf.size(), 0, &z[0], bound, &got) != FLX_OK) return false;
    z.resize(got);
    buf.swap(z);
    return true;
}
// --bam: a piece is STRICT record text (csrc/bam_encode.h: what Emitter::emit_strict appends) with its record offsets; one call
// uploads it, packs the BAM records on the device and compresses them there, so only compressed bytes come back.  Like gz_piece
// it runs on the worker that produced the piece, all workers at once.
static bool bam_piece(flx_bgzf *gz, std::string &buf, const std::vector<uint64_t> &rec_off) {
    const uint64_t n_rec = rec_off.size() - 1;
    if (!gz || n_rec == 0) return buf.empty();
    uint64_t enc = 0, bound = 0, got = 0, bad = 0;
    if (flx_bam_from_fastq_bound(buf.size(), n_rec, &enc) != FLX_OK || flx_bgzf_bound(enc, 0, &bound) != FLX_OK) return false;
    bound += 31 * n_rec;
    std::string z(bound, '\0');
    if (flx_bgzf_bam_from_fastq(gz, buf.data(), buf.size(), rec_off.data(), n_rec, 0, &z[0], bound, &got, &bad) != FLX_OK || bad != n_rec) return false;
    z.resize(got);
    buf.swap(z);
    return true;
}
static const char kBgzfEof[28] = {0x1f, (char)0x8b, 8, 4, 0, 0, 0, 0, 0, (char)0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};

// ---- one read of reads2 as text ------------------------------------------------------------------------------------------
struct Emitter {
    const Reads2 &r2;
    const HeaderOnly &header_only;
    const bool fasta_output, fastq_output;
    // the first passing header-only record without a quality string to repeat: the reference's std::cout dies behind its "+" line
    uint64_t dies_at = UINT64_MAX;
    Emitter(const Reads2 &reads2, const Pass1 &p) : r2(reads2), header_only(p.header_only), fasta_output(p.any_fasta), fastq_output(p.any_fastq) {
        if (fastq_output && !header_only.null_qual.empty())
            for (uint64_t i = 0; i < r2.reads.size() && dies_at == UINT64_MAX; ++i)
                if (r2.pass[i] && !r2.reads[i].child && header_only.null_qual.count(r2.reads[i].rec)) dies_at = i;
    }
    const std::string *repeated_qual(uint64_t i) const {
        if (header_only.stale_qual.empty() || r2.reads[i].child) return nullptr;
        const auto it = header_only.stale_qual.find(r2.reads[i].rec);
        return it == header_only.stale_qual.end() ? nullptr : &it->second;
    }
    void emit(std::string &out, uint64_t i, const Record &r) const {  // output read i of reads2, cut out of its record
        if (!r2.pass[i] || i > dies_at) return;
        const Reads2::Out &o = r2.reads[i];
        if (o.child && o.end - o.start <= 0) return;
        out += fasta_output ? '>' : '@';
        out += o.name;
        if (!r.comment.empty()) { out += ' '; out.append(r.comment.p, r.comment.n); }
        out += '\n';
        out.append(r.seq.p + o.start, (size_t)(o.end - o.start));
        out += '\n';
        if (fastq_output) {
            out += "+\n";
            if (i == dies_at) return;
            if (const std::string *q = repeated_qual(i)) out += *q;
            else out.append(r.qual.p + o.start, (size_t)(o.end - o.start));
            out += '\n';
        }
    }
    // --bam: read i as strict record text and its end in rec_off.  The name goes without its comment (the records carry names
    // only).  A read whose quality line would not have exactly its L bytes (the header-only records above), or holds a byte
    // outside '!'..'~', goes as a FASTA record: its BAM record says "no qualities" (0xFF).  Reads behind dies_at are not written.
    bool written(uint64_t i) const {
        if (!r2.pass[i] || i > dies_at) return false;
        const Reads2::Out &o = r2.reads[i];
        return !(o.child && o.end - o.start <= 0);
    }
    void emit_strict(std::string &out, std::vector<uint64_t> &rec_off, uint64_t i, const Record &r) const {
        if (!written(i)) return;
        const Reads2::Out &o = r2.reads[i];
        const size_t L = (size_t)(o.end - o.start);
        bool with_qual = fastq_output && !fasta_output && i != dies_at && !repeated_qual(i) && r.qual.n == r.seq.n;
        if (with_qual) {
            unsigned out_of_range = 0;
            for (size_t j = 0; j < L; ++j) out_of_range |= (unsigned)((unsigned char)r.qual.p[o.start + j] - 33u > 93u);
            with_qual = !out_of_range;
        }
        out += with_qual ? '@' : '>';
        out += o.name;
        out += '\n';
        out.append(r.seq.p + o.start, L);
        out += '\n';
        if (with_qual) {
            out += "+\n";
            out.append(r.qual.p + o.start, L);
            out += '\n';
        }
        rec_off.push_back(out.size());
    }
    // --bam, a BAM input whose reads go out whole: read i is its record of the inflated input, block_size through the last tag
    void emit_original(std::string &out, const Input &src, uint64_t i) const {
        if (!written(i)) return;
        const uint64_t at = src.bam_rec_at[r2.reads[i].rec];
        out.append(src.owned.data() + at, 4 + (size_t)bam::rd32((const uint8_t *)src.owned.data() + at));
    }
    uint64_t out_bytes(uint64_t i, const Record &r) const {  // what emit appends for read i
        if (!r2.pass[i]) return 0;
        const Reads2::Out &o = r2.reads[i];
        if (o.child && o.end - o.start <= 0) return 0;
        const uint64_t L = (uint64_t)(o.end - o.start);
        if (i > dies_at) return 0;
        uint64_t b = 1 + o.name.size() + (r.comment.empty() ? 0 : 1 + r.comment.n) + 1 + L + 1;
        if (fastq_output) {
            b += 2;
            if (i == dies_at) return b;
            const std::string *q = repeated_qual(i);
            b += (q ? q->size() : L) + 1;
        }
        return b;
    }
    // A passed read whose record in the input already HAS the bytes of its output record — one header line "@name" or
    // "@name comment" with a single blank, one sequence line, a bare "+" line, one quality line, LF ends — is not formatted at
    // all: its bytes go from the mapping [map_lo, map_hi) to the file in one pwritev, neighbours in the input merged into one range.
    // Anything else (children, CRLF, wrapped lines, "+name", tabs) is formatted into a side buffer as before; the byte count per
    // read is the same either way, so the pieces keep their precomputed offsets.
    bool verbatim(uint64_t i, const Record &r, const char *map_lo, const char *map_hi, const char *&from, size_t &len) const {
        if (r2.reads[i].child || i >= dies_at) return false;
        const char *h = r.name.p - 1;
        if (h < map_lo || r.name.p + r.name.n >= map_hi || *h != (fasta_output ? '>' : '@')) return false;
        const char *nl = r.name.p + r.name.n;  // the byte behind the name
        if (!r.comment.empty()) {
            if (*nl != ' ' || r.comment.p != nl + 1 || r.comment.p + r.comment.n >= map_hi) return false;
            nl = r.comment.p + r.comment.n;
        }
        if (*nl != '\n' || r.seq.p != nl + 1 || r.seq.p + r.seq.n >= map_hi || r.seq.p[r.seq.n] != '\n') return false;
        const char *end = r.seq.p + r.seq.n + 1;
        if (fastq_output) {
            if (end + 2 > map_hi || end[0] != '+' || end[1] != '\n' || r.qual.p != end + 2 || r.qual.n != r.seq.n ||
                r.qual.p + r.qual.n >= map_hi || r.qual.p[r.qual.n] != '\n') return false;
            end = r.qual.p + r.qual.n + 1;
        }
        from = h;
        len = (size_t)(end - h);
        return true;
    }
};

// ---- where this rank's records go ----------------------------------------------------------------------------------------
// One rank: straight to stdout.  Several ranks: every rank writes the passed records of its own block to a part file,
// rank 0 streams the parts to stdout in rank (= file) order; or (forked ranks whose common stdout is a regular file) straight
// into that file, each at its own offset.
struct Output {
    FILE *sink = stdout;
    bool shared_file = false, shared_skip = false;  // several ranks, one output file / an earlier rank's output "died": nothing of this rank's follows
    off_t shared_base = -1, shared_end = -1;
    flx_bgzf *gz = nullptr;
    bool pieces_ok = true;
    // --bam (gz is set as well): the file's header, and the BAM input whose records go out as they came in (null: every read is
    // encoded from its text)
    bool bam = false;
    std::string bam_header;
    const Input *bam_original = nullptr;
    // read i of reads2 into a piece under construction, and the piece on its way out
    void emit(const Emitter &em, std::string &buf, std::vector<uint64_t> &rec_off, uint64_t i, const Record &r) const {
        if (!bam) em.emit(buf, i, r);
        else if (bam_original) em.emit_original(buf, *bam_original, i);
        else em.emit_strict(buf, rec_off, i, r);
    }
    bool compress(std::string &buf, const std::vector<uint64_t> &rec_off) const {
        return bam && !bam_original ? bam_piece(gz, buf, rec_off) : gz_piece(gz, buf);
    }
};

static int open_part(const Run &run, Output &out) {
    const std::string path = run.part_path("part", run.rank);
    out.sink = fopen(path.c_str(), "wb");
    if (!out.sink) { std::cerr << "Error: cannot write " << path << "\n"; return 1; }
    return kGoOn;
}

// --bam: a name BAM cannot hold (l_read_name is one byte and counts the NUL) ends the job before anything is written.  Several
// ranks: every rank looks at its own reads, the lowest rank that found one leaves the name where rank 0 reads it.
static int check_bam_names(const Run &run, const Emitter &em) {
    const std::string *bad = nullptr;
    for (uint64_t i = 0; i < em.r2.reads.size() && !bad; ++i)
        if (em.written(i) && (em.r2.reads[i].name.empty() || em.r2.reads[i].name.size() > 254)) bad = &em.r2.reads[i].name;
    std::string name = bad ? *bad : std::string();
    if (run.world > 1) {
        std::vector<uint64_t> found((size_t)run.world, 0);
        found[(size_t)run.rank] = bad != nullptr;
        if (bad && run.rank > 0) {
            FILE *f = fopen(run.part_path("badname", run.rank).c_str(), "wb");
            if (f) { fwrite(name.data(), 1, name.size(), f); fclose(f); }
        }
        if (flx_comm_sum_u64(run.ctx, found.data(), found.size()) != FLX_OK) return run.fail("exchange");
        int first = -1;
        for (int r = run.world - 1; r >= 0; --r)
            if (found[(size_t)r]) first = r;
        if (first < 0) return kGoOn;
        if (run.rank > 0) return 0;  // (rank 0 speaks for the job and gives it its status)
        for (int r = 1; r < run.world; ++r) {
            if (!found[(size_t)r]) continue;
            const std::string pth = run.part_path("badname", r);
            if (r == first)
                if (FILE *f = fopen(pth.c_str(), "rb")) {
                    char buf[4096];
                    size_t got;
                    name.clear();
                    while ((got = fread(buf, 1, sizeof buf, f)) > 0) name.append(buf, got);
                    fclose(f);
                }
            unlink(pth.c_str());
        }
    } else if (!bad) {
        return kGoOn;
    }
    std::cerr << "Error: read name cannot be written as BAM: " << name << "\n";
    return 1;
}

static int begin_output(Run &run, Output &out, const ReadsInput &in, const Pass1 &p, const Emitter &em) {
    const Args &args = run.args;
    if (args.bam) {
        out.bam = true;
        if (in.data.from_bam && in.data.keep_bam) {
            // (the text of record j must be parsed record j: anything else would write some other read's record)
            if (in.streamed || in.data.bam_rec_at.size() != p.kept.recs.size()) {
                if (run.rank == 0) std::cerr << "Error: the records of the BAM input do not match their text\n";
                return run.rank == 0 ? 1 : 0;
            }
            out.bam_original = &in.data;
        }
        if (!out.bam_original)
            if (const int rc = check_bam_names(run, em); rc != kGoOn) return rc;
        if (in.data.from_bam) {
            out.bam_header = in.data.bam_header;
        } else {
            uint64_t len = 0;
            (void)flx_bam_header(nullptr, 0, &len);
            out.bam_header.resize((size_t)len);
            if (flx_bam_header(&out.bam_header[0], len, &len) != FLX_OK) return run.fail("bam header");
        }
    }
    if (run.rank == 0) std::cerr << "Outputting passed long reads\n";
    // (--bam: a piece of ~16 MiB of text ends with the read that crosses that mark; slots with room for it take a piece in one go)
    if ((args.gzip || args.bam) &&
        flx_bgzf_create(run.ctx, args.bam ? 20u << 20 : 16u << 20, (unsigned)std::min<size_t>(host_threads(), 16), &out.gz) != FLX_OK)
        return run.fail(args.bam ? "bam" : "gzip");
    return kGoOn;
}

// --bam: the compressed header in front of rank 0's first piece (a member of its own)
static bool write_bam_header(const Run &run, Output &out) {
    if (!out.bam || run.rank != 0) return true;
    std::string h = out.bam_header;
    return gz_piece(out.gz, h) && fwrite(h.data(), 1, h.size(), out.sink) == h.size();
}

// Round-3 review, item 8: ONE output file.  The ranks forked by --gpus N share the job's stdout; when that is a regular file
// (not in append mode) every rank writes its passed records at its own offset — the sum of the bytes of the ranks in front
// of it, one exchange — with the same pwrite / pwritev pieces a single rank uses, and nothing is written twice.  A pipe, a
// terminal, or ranks under a launcher (no common stdout): part files that rank 0 streams out in order, as before.
static int open_shared_or_part(const Run &run, Output &out, uint64_t my_bytes, bool my_output_dies) {
    const int rank = run.rank, world = run.world;
    std::vector<uint64_t> v(2 + 2 * (size_t)world, 0);
    if (rank == 0 && g_shared_out >= 0 && !getenv("FLX_CLI_ORDERED_OUTPUT") && !out.gz) {  // (--gzip: part files, sizes are not known ahead)
        fflush(stdout);
        struct stat st;
        const int fl = fcntl(g_shared_out, F_GETFL);
        const off_t at = lseek(g_shared_out, 0, SEEK_CUR);
        if (fstat(g_shared_out, &st) == 0 && S_ISREG(st.st_mode) && fl >= 0 && !(fl & O_APPEND) && at >= 0) { v[0] = 1; v[1] = (uint64_t)at; }
    }
    v[2 + (size_t)rank] = my_bytes;
    v[2 + (size_t)world + (size_t)rank] = my_output_dies;
    if (flx_comm_sum_u64(run.ctx, v.data(), v.size()) != FLX_OK) return run.fail("exchange");
    if (!v[0] || g_shared_out < 0) return open_part(run, out);
    out.shared_file = true;
    uint64_t before = 0, total = 0;
    bool dead = false;
    for (int r = 0; r < world; ++r) {
        if (r == rank) { before = total; out.shared_skip = dead; }
        if (!dead) total += v[2 + (size_t)r];
        dead = dead || v[2 + (size_t)world + (size_t)r] != 0;
    }
    out.shared_base = (off_t)(v[1] + before);
    out.shared_end = (off_t)(v[1] + total);
    out.sink = fdopen(dup(g_shared_out), "wb");
    return out.sink ? kGoOn : write_error();
}

// ---- a mapped input --------------------------------------------------------------------------------------------------------
// One piece of the output written by its producer: ranges of the mapping and formatted records interleaved, pwritev at `at`.
struct PieceWriter {
    const int fd;
    off_t at;
    std::vector<struct iovec> iov;
    std::deque<std::string> side;
    bool last_is_map = false;
    bool flush() {
        size_t k = 0;
        while (k < iov.size()) {
            const int cnt = (int)std::min<size_t>(iov.size() - k, 512);
            ssize_t w = pwritev(fd, iov.data() + k, cnt, at);
            if (w <= 0) return false;
            at += w;
            while (w > 0 && k < iov.size()) {  // a short write: drop what went out
                if ((size_t)w >= iov[k].iov_len) { w -= (ssize_t)iov[k].iov_len; ++k; }
                else { iov[k].iov_base = (char *)iov[k].iov_base + w; iov[k].iov_len -= (size_t)w; w = 0; }
            }
        }
        iov.clear();
        side.clear();
        last_is_map = false;
        return true;
    }
    void from_map(const char *from, size_t len) {
        if (last_is_map && (const char *)iov.back().iov_base + iov.back().iov_len == from) iov.back().iov_len += len;  // neighbours in the input
        else iov.push_back({(void *)from, len});
        last_is_map = true;
    }
    std::string &formatted() { side.emplace_back(); return side.back(); }
    void take_formatted() {
        if (side.back().empty()) return;
        iov.push_back({(void *)side.back().data(), side.back().size()});
        last_is_map = false;
    }
};

// reads2 [first, last) of a mapped input into the regular file `fd` at [at, at_end); true: exactly those bytes were written
static bool pwritev_piece(const Emitter &em, const std::vector<Record> &recs, const Input &data, uint64_t first, uint64_t last, int fd,
                          off_t at, off_t at_end) {
    const char *map_lo = data.data(), *map_hi = data.data() + data.size();
    PieceWriter w{fd, at, {}, {}};
    for (uint64_t i = first; i < last; ++i) {
        if (!em.r2.pass[i]) continue;
        const Record &r = recs[em.r2.reads[i].rec];
        const char *from = nullptr;
        size_t len = 0;
        if (em.verbatim(i, r, map_lo, map_hi, from, len)) {
            w.from_map(from, len);
        } else {
            em.emit(w.formatted(), i, r);
            w.take_formatted();
        }
        if (w.iov.size() >= 4096 && !w.flush()) return false;
    }
    return w.flush() && w.at == at_end;
}

// The passed records are cut out of the mapped input by several threads, ~16 MiB of output per piece.  Every piece's
// place in the output is known beforehand, so when the sink is a regular file each thread writes its pieces itself
// (pwrite at the piece's offset); a pipe or terminal gets the pieces in order from this thread.
static int write_output_mapped(const Run &run, const ReadsInput &in, const Pass1 &p, const Emitter &em, Output &out) {
    const std::vector<Record> &recs = p.kept.recs;
    const Reads2 &r2 = em.r2;
    const uint64_t n2 = r2.reads.size();
    std::vector<uint64_t> piece_first{0}, piece_at{0};  // reads2 range and byte offset of every piece
    {
        uint64_t bytes = 0, in_piece = 0;
        for (uint64_t i = 0; i < n2; ++i) {
            const uint64_t b = em.out_bytes(i, recs[r2.reads[i].rec]);
            bytes += b;
            in_piece += b;
            if (in_piece >= (16u << 20) && i + 1 < n2) { piece_first.push_back(i + 1); piece_at.push_back(bytes); in_piece = 0; }
        }
        piece_first.push_back(n2);
        piece_at.push_back(bytes);
    }
    if (run.world > 1)
        if (const int rc = open_shared_or_part(run, out, piece_at.back(), em.dies_at != UINT64_MAX); rc != kGoOn) return rc;
    const char *fail_env = getenv("FLX_CLI_FAIL_WRITE_RANK");  // tests: this rank's writes fail (a full disk under one rank's share of the file)
    const bool fail_writes = fail_env && atoi(fail_env) == run.rank;
    const bool ok = out.shared_skip || (write_bam_header(run, out) && write_pieces(piece_first.size() - 1, [&](size_t j, std::string &buf, const PieceTarget &to) {
        if (fail_writes) return false;
        if (!to.direct) {  // a pipe / terminal / append-mode file: the caller writes the formatted piece in order
            std::vector<uint64_t> rec_off{0};
            for (uint64_t i = piece_first[j]; i < piece_first[j + 1]; ++i) out.emit(em, buf, rec_off, i, recs[r2.reads[i].rec]);
            return out.compress(buf, rec_off);
        }
        // regular file: this thread writes the piece itself
        buf.clear();
        return pwritev_piece(em, recs, in.data, piece_first[j], piece_first[j + 1], to.fd, to.base + (off_t)piece_at[j], to.base + (off_t)piece_at[j + 1]);
    }, out.sink, out.gz ? nullptr : &piece_at, out.shared_file ? out.shared_base : (off_t)-1));  // (--gzip, --bam: formatted and compressed, in order)
    // (several ranks: a rank that could not write — a full disk under its pwrite — still goes to the exchange of finish_output, where
    // every rank learns of it and rank 0 says why; leaving here would strand the others in that exchange)
    if (!ok && run.world == 1) return write_error();
    out.pieces_ok = ok;
    return kGoOn;
}

// ---- a streamed input ------------------------------------------------------------------------------------------------------
// Second pass over the compressed input (src/main.cpp:263-313 re-reads the file too), but not front to back on one
// thread: pass 1 left access points in the deflate stream, the pieces between them (whole records, ~32 MiB of text)
// are inflated and parsed concurrently and written in order.  Pieces without a passing read are not inflated at all.
static int write_output_streamed(const Run &run, const ReadsInput &in, const Pass1 &p, const Emitter &em, Output &out) {
    if (run.world > 1)  // (several ranks: every rank's records to its part file, rank 0 streams the parts out in order: finish_output)
        if (const int rc = open_part(run, out); rc != kGoOn) return rc;
    const Reads2 &r2 = em.r2;
    const UnitIndex &units = p.units;
    const uint64_t n2 = r2.reads.size(), n = p.lengths.size();
    const size_t n_units = units.units();
    std::vector<uint64_t> r2_at(n_units + 1, n2);  // first reads2 entry of every unit (reads2 is in record order)
    {
        uint64_t cur = 0;
        for (size_t j = 0; j < n_units; ++j) {
            while (cur < n2 && r2.reads[cur].rec < units.first_rec[j]) ++cur;
            r2_at[j] = cur;
        }
    }
    const bool ok = write_bam_header(run, out) && write_pieces(n_units, [&](size_t j, std::string &buf, const PieceTarget &) {
        bool any = false;
        for (uint64_t i = r2_at[j]; i < r2_at[j + 1] && !any; ++i) any = r2.pass[i] != 0;
        if (!any) return true;
        std::vector<char> text;
        Parsed got;
        if (!inflate_range(in.blocks.file, in.blocks.points[j], units.start[j], units.start[j + 1], text)) return false;
        Input view;
        view.p = text.data();
        view.n = text.size();
        parse_sequential(view, got);
        if (got.recs.size() != units.first_rec[j + 1] - units.first_rec[j]) return false;
        uint64_t cur = r2_at[j];
        std::vector<uint64_t> rec_off{0};
        for (size_t k = 0; k < got.recs.size(); ++k) {
            const uint64_t rec = units.first_rec[j] + k;
            const Record &r = got.recs[k];
            if (rec < p.lo_rec || rec - p.lo_rec >= n) continue;  // (several ranks: a unit at the edge of the share holds other ranks' records too)
            if (r.name.sv() != p.names[rec - p.lo_rec] || (int32_t)r.seq.size() != p.lengths[rec - p.lo_rec]) return false;
            for (; cur < r2_at[j + 1] && r2.reads[cur].rec == rec; ++cur) out.emit(em, buf, rec_off, cur, r);
        }
        return out.compress(buf, rec_off);
    }, out.sink, nullptr);
    if (g_gpu_inflater.output_pass && getenv("FLX_CLI_PINFLATE_TIMING"))
        fprintf(stderr, "[pinflate] device: output pass: %llu units inflated on the device, %llu by zlib\n",
                (unsigned long long)g_gpu_inflater.out_device.load(), (unsigned long long)g_gpu_inflater.out_zlib.load());
    if (!ok && run.world == 1) { std::cerr << "Error: " << run.args.input_reads << " could not be read a second time (did it change?)\n"; return 1; }
    out.pieces_ok = ok;  // (several ranks: to the exchange of finish_output, like a failed write)
    return kGoOn;
}

// ---- the end of the output pass ----------------------------------------------------------------------------------------------
// several ranks, part files: rank 0 streams them to stdout in rank (= file) order; done[r + 1]: the output of rank r "died"
static int stitch_rank_outputs(const Run &run, const std::vector<uint64_t> &done) {
    std::vector<char> buf(1 << 22);
    bool dead = false;
    for (int r = 0; r < run.world; ++r) {
        const std::string pth = run.part_path("part", r);
        if (dead) { unlink(pth.c_str()); continue; }
        dead = done[(size_t)r + 1] != 0;
        FILE *f = fopen(pth.c_str(), "rb");
        if (!f) { std::cerr << "Error: cannot read " << pth << "\n"; return 1; }
        size_t got;
        bool wrote = true;
        while (wrote && (got = fread(buf.data(), 1, buf.size(), f)) > 0) wrote = fwrite(buf.data(), 1, got, stdout) == got;
        fclose(f);
        unlink(pth.c_str());
        if (!wrote) {
            for (int q = r + 1; q < run.world; ++q) unlink(run.part_path("part", q).c_str());
            return write_error();
        }
    }
    if (((run.args.gzip || run.args.bam) && fwrite(kBgzfEof, 1, 28, stdout) != 28) || fflush(stdout) != 0) return write_error();
    return kGoOn;
}

static int finish_output(const Run &run, Output &out, const Emitter &em) {
    const int rank = run.rank, world = run.world;
    // a sink that did not take everything (disk full, the reader of a pipe gone while SIGPIPE is ignored) ends the job with status 1
    const bool sink_ok = out.pieces_ok && (!out.gz || world > 1 || fwrite(kBgzfEof, 1, 28, out.sink) == 28) && fflush(out.sink) == 0 && !ferror(out.sink);
    flx_bgzf_destroy(out.gz);
    out.gz = nullptr;
    if (world == 1) return sink_ok ? kGoOn : write_error();
    fclose(out.sink);
    // every part is complete before rank 0 reads it; a rank whose output "died" (Emitter) ends the whole output
    std::vector<uint64_t> done((size_t)world + 1, 0);
    done[0] = sink_ok;
    done[(size_t)rank + 1] = em.dies_at != UINT64_MAX;
    if (flx_comm_sum_u64(run.ctx, done.data(), done.size()) != FLX_OK) return run.fail("exchange");
    if (done[0] != (uint64_t)world) {  // some rank could not write its share: every rank leaves, rank 0 says why
        if (rank == 0) {
            for (int r = 0; r < world && !out.shared_file; ++r) unlink(run.part_path("part", r).c_str());
            return write_error();
        }
        return 0;
    }
    if (out.shared_file) {  // everything is in the file already (every rank has written when the exchange returns): the position behind it
        if (rank == 0 && lseek(g_shared_out, out.shared_end, SEEK_SET) < 0) return write_error();
    } else if (rank == 0) {
        return stitch_rank_outputs(run, done);
    }
    return kGoOn;
}
