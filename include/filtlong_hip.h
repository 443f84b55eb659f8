/* filtlong_hip.h — C ABI of the MI355X-native Filtlong scoring hot path.
 *
 * This is the drop-in boundary: a C-ABI shared library (libfiltlong_hip.so, gfx950) whose entry
 * points replace, in batched form, the in-process seams of the reference (rrwick/Filtlong v0.3.1;
 * paths below are relative to the reference root):
 *
 *   seam 1  reference 16-mer set build      Kmers::Kmers / add_assembly_fasta / add_read_fastqs /
 *                                           is_kmer_present / empty        src/kmers.h:31-44
 *   seam 2  per-read scoring                Read::Read(name, seq, qscores, length, Kmers*, Arguments*)
 *                                           and its public result fields   src/read.h:32-56
 *   seam 3  global rank + cut               the statistics / normalise / set_final_score /
 *                                           std::sort / cut walk inlined in main()
 *                                                                          src/main.cpp:169-261
 *
 * Conventions
 *   - plain pointers and sizes only; no C++ or torch types cross the boundary;
 *   - every function returns an int status (FLX_OK == 0); no exceptions cross the boundary;
 *     flx_last_error(ctx) gives the message (the CLI prints it as "Error: ..." and exits 1,
 *     mirroring src/main.cpp:80-116);
 *   - one flx_ctx per process / rank / GPU; not thread-safe; calls are synchronous on return
 *     unless the name ends in _async;
 *   - `*_dev` variants take DEVICE pointers (HBM-resident data, e.g. a torch tensor's data_ptr())
 *     and run on the context's stream; the plain variants take HOST pointers and stage through
 *     the context's own device buffers;
 *   - there is NO CPU fallback: if the HIP runtime or a gfx950 device is missing,
 *     flx_ctx_create fails.
 */
#ifndef FILTLONG_HIP_H
#define FILTLONG_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2 (round 4): + flx_device_count, flx_reads2_gather(_dev) (added in round 3 under version 1), flx_last_kmer_locus; finalize of a
 * set built from an assembly also keeps the assembly as a text + seed table (0.5 B per base + 10 B per distinct 16-mer of device
 * memory beside the 512 MiB bitmap, 1 GiB pair table and 2 + 2 MiB prefilters); when that memory cannot be had the set works without */
/* 3 (round 5): + flx_last_kmer_fold_grid */
/* 4 (round 6): + flx_last_kmer_cover, flx_last_kmer_handed_over, flx_synth_seq_profile_dev; added under version 4: the BGZF
 * compressor (flx_bgzf_bound, flx_bgzf_compress_dev, flx_bgzf_create / _compress / _destroy), the read summary
 * (flx_summary_q_edges, flx_summary_dev, flx_summary), the BGZF inflater (flx_bgzf_index, flx_bgzf_inflate_dev,
 * flx_bgzf_inflate), the BAM reader (flx_bam_index, flx_bam_to_fastq_dev, flx_bam_to_fastq) and the BAM writer (flx_bam_header,
 * flx_bam_from_fastq_bound, flx_bam_from_fastq_dev, flx_bgzf_bam_from_fastq) */
#define FLX_ABI_VERSION 4

enum flx_status {
    FLX_OK = 0,
    FLX_ERR_INVALID = 1,     /* bad argument                                  */
    FLX_ERR_HIP = 2,         /* HIP runtime error (message has the hipError)   */
    FLX_ERR_NOMEM = 3,       /* host or device allocation failed              */
    FLX_ERR_STATE = 4,       /* call order violated (e.g. set not finalized)  */
    FLX_ERR_CAPACITY = 5,    /* caller-provided output capacity too small     */
    FLX_ERR_NO_DEVICE = 6,   /* no usable gfx950 device                       */
    FLX_NEED_REPLICATED = 100 /* flx_rank_and_cut_sharded_dev only: not an error — nothing was modified; gather all
                                records and call flx_rank_and_cut_dev instead (NaN scores / ties straddling the cut) */
};

typedef struct flx_ctx flx_ctx;
typedef struct flx_kmerset flx_kmerset;
typedef struct flx_adapters flx_adapters;

/* Hot-path parameters: the fields of the reference's Arguments that Read::Read consults
 * (src/arguments.h:59-91; read in src/read.cpp:61-73,86-117).  *_set mirrors the reference's
 * paired bools. */
typedef struct flx_params {
    int32_t window_size;                  /* --window_size, default 250 (src/arguments.cpp:205)   */
    int32_t min_length_set, min_length;   /* --min_length                                          */
    int32_t max_length_set, max_length;   /* --max_length                                          */
    int32_t min_mean_q_set;               /* --min_mean_q                                          */
    int32_t min_window_q_set;             /* --min_window_q                                        */
    double min_mean_q;
    double min_window_q;
    int32_t trim;                         /* --trim                                                */
    int32_t split_set, split;             /* --split                                               */
    int32_t _pad;
} flx_params;

/* ------------------------------------------------------------------------------------------
 * context
 * ---------------------------------------------------------------------------------------- */
int flx_abi_version(void);
const char *flx_version(void);
/* Number of HIP devices visible to this process (-1: no usable runtime).  Initialises the HIP runtime in the calling process:
 * a host that forks its ranks (the CLI's --gpus N) asks from a short-lived probe child. */
int flx_device_count(void);
int flx_ctx_create(int device_ordinal, flx_ctx **out);
void flx_ctx_destroy(flx_ctx *ctx);
const char *flx_last_error(const flx_ctx *ctx); /* ctx may be NULL: last create error */
/* Run all subsequent work of this context on the caller's hipStream_t (NULL = context's own). */
int flx_ctx_set_stream(flx_ctx *ctx, void *hip_stream);
int flx_ctx_synchronize(flx_ctx *ctx);
/* Device properties the host side reports (name is copied, NUL-terminated). */
int flx_ctx_device_info(const flx_ctx *ctx, char *name, size_t name_cap, int *n_cu, uint64_t *hbm_bytes);

/* Per-kernel timing with HIP events on the context's stream (for bench.py's roofline line).
 * While enabled, every launch of a hot kernel is bracketed by events; flx_timing_get drains them
 * (synchronising) and returns total milliseconds and launch count for kernels whose name starts
 * with `prefix` ("" = all). */
/* Name of the Phred scoring kernel the last Phred-mode scoring call launched (the library picks by window size and data:
 * "flx_score_phred_regs", "flx_score_phred_regs_private", "flx_score_phred_ring" or "flx_score_phred_direct"). */
const char *flx_last_phred_kernel(const flx_ctx *ctx);
/* 1 when the last k-mer-mode scoring call confirmed members along the reads' loci in the assembly text (sets built from an
 * assembly; FLX_KMER_LOCUS=0 switches it off), 0 otherwise.  Results are identical either way. */
int flx_last_kmer_locus(const flx_ctx *ctx);
/* 1 when the window recurrence of the last k-mer-mode scoring call ran on the integer grid (exact; window sizes whose step 1 / ws
 * rounds alike on the binades from 2^-3 to 2 — the default 250 among them; FLX_KMER_FOLD_GRID=0 switches it off), 0 when every step
 * was taken in floating point.  Results are identical either way. */
int flx_last_kmer_fold_grid(const flx_ctx *ctx);
/* Which coverage kernel the last k-mer-mode scoring call launched: "q" (phases with a queue in LDS between them, the default for a
 * set with a text), "q2" (FLX_KMER_COVER=q2: the same with every read in its second launch, tests), "w" (the wave-level kernel of rounds
 * 3-5: sets without a text, FLX_KMER_COVER=w) or "v2" (FLX_KMER_COVER=v2, sets without the pair table).  Results are identical whichever runs. */
const char *flx_last_kmer_cover(const flx_ctx *ctx);
/* How many reads of the last k-mer-mode scoring call the first coverage kernel handed to the one in which every lane follows a
 * diagonal of its own (reads with insertions / deletions; kernel "q" only, 0 otherwise; valid until the next scoring call of the
 * context; a device-to-host copy of one byte per read: for tests and diagnostics).  -1 on error. */
int64_t flx_last_kmer_handed_over(flx_ctx *ctx);
int flx_timing_enable(flx_ctx *ctx, int on);
int flx_timing_reset(flx_ctx *ctx);
int flx_timing_get(flx_ctx *ctx, const char *prefix, double *total_ms, uint64_t *launches);

/* ------------------------------------------------------------------------------------------
 * seam 2 — per-read scoring      (replaces Read::Read, src/read.cpp:25-144)
 *
 * Packed input ("read plane"): one byte plane + per-read start offsets + lengths.
 *   - Phred mode (set == NULL or empty): plane holds the QUALITY strings (the reference never
 *     touches seq in this mode, src/read.cpp:35-39);
 *   - k-mer mode: plane holds the SEQUENCE strings (qual is never touched, src/read.cpp:43-58).
 *   - offsets[i] must be a multiple of 16 and plane_bytes a multiple of 16 covering
 *     offsets[i] + round_up(lengths[i], 16) for every read (flx_plane_layout computes both).
 *   - `order` (optional, may be NULL) is a permutation of [0, n): the processing order; pass the
 *     reads sorted by DESCENDING length (flx_length_order) so that the 64 reads sharing a wavefront
 *     finish together.  Results are always written in input order (index i = read i).
 *
 * Outputs per read i: mean_q, window_q (the 0-100 pre-normalisation values of m_mean_quality /
 * m_window_quality), passed (m_passed after the hard cut-offs, src/read.cpp:64-73), and in k-mer
 * mode first/last (m_first_base_in_kmer / m_last_base_in_kmer, src/read.cpp:75-84) plus the child
 * reads produced by --trim/--split (src/read.cpp:86-141) in CSR form: children of read i are
 * child_offsets[i] .. child_offsets[i+1]-1, each with its half-open 0-based (start,end) range and
 * its own mean_q / window_q / passed.
 * ---------------------------------------------------------------------------------------- */
typedef struct flx_scores {
    double *mean_q;          /* [n]                                   */
    double *window_q;        /* [n]                                   */
    uint8_t *passed;         /* [n]                                   */
    int32_t *first;          /* [n] or NULL (k-mer mode only)         */
    int32_t *last;           /* [n] or NULL                           */
    uint64_t *child_offsets; /* [n+1] or NULL (trim/split only)       */
    int32_t *child_ranges;   /* [2*child_capacity] (start,end) pairs  */
    double *child_mean_q;    /* [child_capacity]                      */
    double *child_window_q;  /* [child_capacity]                      */
    uint8_t *child_passed;   /* [child_capacity]                      */
    uint64_t child_capacity; /* in: capacity of the child arrays      */
    uint64_t n_children;     /* out: total children written           */
} flx_scores;

/* Layout helper: offsets[i] (16-byte aligned starts) and the padded plane size for given lengths. */
int flx_plane_layout(const int32_t *lengths, uint64_t n_reads, uint64_t *offsets, uint64_t *plane_bytes);
/* Processing order: indices sorted by descending length (stable). Host arrays. */
int flx_length_order(const int32_t *lengths, uint64_t n_reads, uint32_t *order);

int flx_score_batch(flx_ctx *ctx, const flx_kmerset *set, const uint8_t *plane, uint64_t plane_bytes,
                    const uint64_t *offsets, const int32_t *lengths, const uint32_t *order, uint64_t n_reads,
                    const flx_params *params, flx_scores *out);

/* Device-resident variant: every pointer (including those inside `out`) is a device pointer. */
int flx_score_batch_dev(flx_ctx *ctx, const flx_kmerset *set, const void *d_plane, uint64_t plane_bytes,
                        const void *d_offsets, const void *d_lengths, const void *d_order, uint64_t n_reads,
                        const flx_params *params, flx_scores *out_dev);

/* ------------------------------------------------------------------------------------------
 * seam 2, Phred mode with --split_window_q (added under version 4; the reference has no counterpart: its --trim / --split need
 * an external reference and --min_window_q drops the whole read): reads are split at their low-quality windows.  Defined on
 * integers, so every decomposition gives the same answer:
 *   E[b], uint32, for quality byte b: q = (signed char)b - 33; 2^32 - 1 for q <= 0, else min(2^32 - 1, floor(10^(-q/10) 2^32 + 0.5))
 *   t = (uint64_t)floor((100 - Q) / 100 * 2^32) in IEEE double, 0 < Q < 100 on the scale of --min_window_q
 *   with W = params->window_size, L the read's length and n = min(W, L): the window ending at base j, n - 1 <= j < L, is bad iff
 *   the sum of E over bases j - n + 1 .. j is > t * n (uint64).  Every base inside a bad window is removed; a child is a maximal
 *   run of the bases left, (start, end) half-open and 0-based.
 * The plane holds the QUALITY strings, laid out as for flx_score_batch.  A read keeps the mean_q / window_q of flx_score_batch; a
 * child gets the bits flx_score_batch gives its quality substring as a read of its own, and its pass flag from the hard cut-offs
 * applied to it.  A read without a bad window has no children and goes on as itself; one with bad windows and no base left has no
 * children and passed = 0.  first / last (when not NULL) hold the first kept base and one past the last: 0 and L without a bad
 * window, -1 and -1 when nothing is kept.  out->child_offsets is required; FLX_ERR_CAPACITY as for --trim / --split
 * (out->n_children is then the capacity needed).  params->trim and params->split_set must be 0.
 *   flx_qsplit_table / flx_qsplit_threshold   host only, no device: E and t (FLX_ERR_INVALID unless 0 < q < 100)
 * ---------------------------------------------------------------------------------------- */
int flx_qsplit_table(uint32_t e[256]);
int flx_qsplit_threshold(double q, uint64_t *t);
int flx_score_batch_qsplit(flx_ctx *ctx, const uint8_t *plane, uint64_t plane_bytes, const uint64_t *offsets,
                           const int32_t *lengths, const uint32_t *order, uint64_t n_reads, const flx_params *params,
                           double split_window_q, flx_scores *out);
int flx_score_batch_qsplit_dev(flx_ctx *ctx, const void *d_plane, uint64_t plane_bytes, const void *d_offsets,
                               const void *d_lengths, const void *d_order, uint64_t n_reads, const flx_params *params,
                               double split_window_q, flx_scores *out_dev);

/* ------------------------------------------------------------------------------------------
 * the contaminant screen (added under version 4; the reference has no counterpart: its users run NanoLyse or chopper --contam over
 * the whole file in front of it): how many 16-mers of every read are members of a set X built from a contaminant — the lambda control
 * strand, a vector, a phage, an organelle.  Defined on integers, so every decomposition gives the same answer:
 *   X          every 16-mer of both strands of the contaminant that consists of ACGTacgt only.  flx_screen_set_add cuts every
 *              sequence at each byte outside ACGTacgt and hands the pieces of at least 16 bases to flx_kmerset_add_assembly as
 *              sequences of their own (flx_kmerset_add_assembly encodes any other byte as A, like the reference: an N run would put
 *              poly-A into X); flx_kmerset_finalize follows as usual.  16-mers cannot screen a large genome: an unrelated read
 *              keeps |X| / 2^32 of its windows.
 *   hits[i]    with windows = max(0, L - 15) for a read of L bases: the number of positions p in [0, windows) whose 16 bytes are all
 *              in ACGTacgt and whose forward 2-bit code (A 0, C 1, G 2, T 3, first base on top: flx_kmerset_contains) is in X
 *   t          flx_screen_threshold: (uint64_t)ceil(P / 100 * 2^32) in IEEE double; FLX_ERR_INVALID unless 0 < P <= 100.  Host only.
 *   excluded   iff windows > 0 and ((uint64_t)hits << 32) >= t * windows
 * flx_screen_hits(_dev): the plane holds SEQUENCES, laid out as for flx_score_batch; `order` may be NULL; hits has n_reads entries
 * (_dev: every pointer is a device pointer and the call returns with the work queued on the context's stream).  FLX_ERR_STATE for a
 * set that is empty or not finalized.  The work item is a span of flx_screen_span() window positions of one read (host only: tests
 * place lengths on its edges), so one very long read spreads over the whole device.  Timed as "flx_screen".
 * flx_last_screen_filter: which filter stood in front of the exact bitmap in the last call — "lds" (the 10-mers of X in the LDS of
 * every CU, then the 12-mer prefilter: sets filled through flx_screen_set_add whose 10-mer table is at most seven eighths full),
 * "pre12" (the 12-mer prefilter alone; FLX_KMER_PREFILTER=12 asks for it, =10 for "lds" however full the table) or "exact" (no
 * prefilter: FLX_KMER_PREFILTER=0, or a set too large for one).  The hits are the
 * same whichever runs.
 * ---------------------------------------------------------------------------------------- */
int flx_screen_threshold(double percent, uint64_t *t);
uint32_t flx_screen_span(void);
int flx_screen_set_add(flx_kmerset *set, const uint8_t *bases, const uint64_t *offsets, const int64_t *lengths, uint64_t n_seqs);
int flx_screen_hits(flx_ctx *ctx, const flx_kmerset *set, const uint8_t *plane, uint64_t plane_bytes, const uint64_t *offsets,
                    const int32_t *lengths, const uint32_t *order, uint64_t n_reads, uint32_t *hits);
int flx_screen_hits_dev(flx_ctx *ctx, const flx_kmerset *set, const void *d_plane, uint64_t plane_bytes, const void *d_offsets,
                        const void *d_lengths, const void *d_order, uint64_t n_reads, uint32_t *d_hits);
const char *flx_last_screen_filter(const flx_ctx *ctx);

/* ------------------------------------------------------------------------------------------
 * the screen with K-mers of 16 <= K <= 31 bases (added under version 4): what lets --exclude screen a genome.  The definition above
 * with 16 replaced by K: windows = max(0, L - K + 1), a window counts if its K bytes are all in ACGTacgt and it is in X_K, every K-mer
 * of either strand of the reference that consists of ACGTacgt only (no window spans two sequences); t and the decision are unchanged.
 * A window's forward code has A 0, C 1, G 2, T 3, the first base on top, in 2 K bits; the set stores CANONICAL keys, the smaller of a
 * window's code and its reverse complement's, in an open-addressing table of 64-bit slots in device memory: capacity a power of two
 * and at least twice the stored keys after every add, linear probing.  Neither the hash nor the capacity can change a result.
 *   flx_screenset_create    k outside 16..31 or a hint outside 1..40: FLX_ERR_INVALID.  The table starts at 2^log2_capacity_hint slots;
 *                           it grows (every key is rehashed) before a batch whose windows could take the load above 1/2, so a caller
 *                           who knows the reference's size passes log2 of twice its bases and the table is never rehashed.
 *   flx_screenset_add       host arrays, any offsets, sequences back to back; lengths up to 2^31 - 1 (FLX_ERR_INVALID beyond); any
 *                           number of calls.  Nothing is cut on the host: a window with a byte outside ACGTacgt is not valid.
 *   flx_screenset_finalize  afterwards every call but the getters and flx_screenset_destroy is FLX_ERR_STATE
 *   flx_screenset_size      the stored canonical keys;  flx_screenset_k, flx_screenset_capacity (slots of 8 bytes)
 *   flx_screenset_hits(_dev) arguments, checks and timing name of flx_screen_hits(_dev); flx_last_screen_filter then answers "hash"
 * A device allocation that fails is FLX_ERR_NOMEM and leaves the set as it was before the call.
 * ---------------------------------------------------------------------------------------- */
typedef struct flx_screenset flx_screenset;
int flx_screenset_create(flx_ctx *ctx, int k, int log2_capacity_hint, flx_screenset **out);
int flx_screenset_add(flx_screenset *set, const uint8_t *bases, const uint64_t *offsets, const int64_t *lengths, uint64_t n_seqs);
int flx_screenset_finalize(flx_screenset *set);
uint64_t flx_screenset_size(const flx_screenset *set);
int flx_screenset_k(const flx_screenset *set);
uint64_t flx_screenset_capacity(const flx_screenset *set);
void flx_screenset_destroy(flx_screenset *set);
int flx_screenset_hits(flx_ctx *ctx, const flx_screenset *set, const uint8_t *plane, uint64_t plane_bytes, const uint64_t *offsets,
                       const int32_t *lengths, const uint32_t *order, uint64_t n_reads, uint32_t *hits);
int flx_screenset_hits_dev(flx_ctx *ctx, const flx_screenset *set, const void *d_plane, uint64_t plane_bytes, const void *d_offsets,
                           const void *d_lengths, const void *d_order, uint64_t n_reads, uint32_t *d_hits);

/* ------------------------------------------------------------------------------------------
 * the low-complexity filter (added under version 4; the reference has no counterpart: its users run fastp -y, prinseq -lc_method dust
 * or an entropy filter over the whole file in front of it): how many 64-base windows of every read are simple repeats.  Defined on
 * integers, so every decomposition gives the same answer:
 *   window     64 consecutive bases = 62 overlapping triplets; a read of L bases has windows = max(0, L - 63), one per start position
 *   c_t        for a window whose 64 bytes are all in ACGTacgt (case folded; A 0, C 1, G 2, T 3): how often triplet kind t of the 64
 *              kinds occurs among the window's 62 triplets
 *   S          sum over t of c_t (c_t - 1) / 2, the pairs of equal triplets, 0 .. 1891: the score of DUST / sdust at one fixed
 *              window length
 *   bad window all 64 bytes in ACGTacgt AND 10 S > score_t * 61; score_t is an integer on sdust's scale of tenths, 10 .. 300
 *              (20 is sdust's default).  Equality is not bad: at 20, S = 122 is good and S = 123 is bad.  A window with any other
 *              byte is never bad.
 *   flagged    iff windows > 0 and ((uint64_t)bad << 32) >= t * windows, t = flx_screen_threshold(percent): the screen's rule
 * flx_complexity_bad(_dev): the arguments and checks of flx_screen_hits(_dev) without the set; bad has n_reads entries and is not
 * accumulated across calls.  FLX_ERR_INVALID for score_t outside 10..300.  The work item is a span of flx_complexity_span() window
 * start positions of one read (a multiple of flx_complexity_window() = 64; host only: tests place lengths on its edges), every lane
 * of a wave walking span / 64 of them from a fresh state.  Timed as "flx_complexity".
 * ---------------------------------------------------------------------------------------- */
uint32_t flx_complexity_window(void);
uint32_t flx_complexity_span(void);
int flx_complexity_bad(flx_ctx *ctx, const uint8_t *plane, uint64_t plane_bytes, const uint64_t *offsets, const int32_t *lengths,
                       const uint32_t *order, uint64_t n_reads, int score_t, uint32_t *bad);
int flx_complexity_bad_dev(flx_ctx *ctx, const void *d_plane, uint64_t plane_bytes, const void *d_offsets, const void *d_lengths,
                           const void *d_order, uint64_t n_reads, int score_t, uint32_t *d_bad);

/* ------------------------------------------------------------------------------------------
 * adapter trimming (added under version 4; the reference has no counterpart: its users run an adapter trimmer over the whole file
 * in front of it): known adapters are cut off the two ends of every read.  Defined on integers, so every decomposition gives the
 * same answer:
 *   patterns   every sequence handed to flx_adapters_create, upper-cased, and its reverse complement: pattern 2 i is sequence i,
 *              pattern 2 i + 1 its reverse complement.  12 to 64 bases of ACGT each, at most 128 sequences.  A pattern of m bases may
 *              carry k = m * E / 100 edits (integer division), E = errors_percent, 0..40.
 *   texts      W = window, 1..1024; n = min(L, W) for a read of L bases.  The head text is read[0, n); the tail text is
 *              read[L - n, L) reversed, matched against the patterns reversed.  Lower case is folded; a byte outside ACGTacgt
 *              equals no pattern base.
 *   match      unit-cost edit distance of the whole pattern against any substring of the text: D[0][j] = 0, D[i][0] = i,
 *              d(j) = D[m][j], 1 <= j <= n; dmin = min d(j), jbest the largest j with d(j) = dmin; a hit iff n >= 1 and dmin <= k.
 *   keys       per read end, max over the hitting patterns of (jbest << 8) | pattern; 0 without a hit.  cut = key >> 8.
 *   children   s = cut_head, e = L - cut_tail.  No hit at either end: the read goes on as itself, no children, first = 0, last = L.
 *              s < e: one child [s, e).  s >= e: no children, first = last = -1 and passed = 0.
 * flx_adapters_create: FLX_ERR_INVALID for a sequence outside 12..64 bases or not ACGT, no sequence or more than 128, E outside
 * 0..40 or W outside 1..1024.  The object belongs to no context; a device gets its copy of the patterns with the first call there.
 * flx_adapter_cuts(_dev): the plane holds SEQUENCES, laid out as for flx_score_batch; `order` may be NULL; keys has 2 * n_reads
 * entries, head and tail of read i at 2 i and 2 i + 1 (_dev: every pointer is a device pointer and the call returns with the work
 * queued on the context's stream).  Timed as "flx_adapters".
 * flx_score_batch_adapters(_dev): the quality plane and the sequence plane share offsets and lengths.  A read keeps the mean_q /
 * window_q of flx_score_batch; a child gets the bits flx_score_batch gives its quality substring and its own hard cut-offs.
 * first / last, child_offsets and FLX_ERR_CAPACITY as for flx_score_batch_qsplit.  params->trim and params->split_set must be 0.
 * ---------------------------------------------------------------------------------------- */
int flx_adapters_create(const uint8_t *bases, const uint64_t *offsets, const int64_t *lengths, uint64_t n_seqs, int errors_percent,
                        int window, flx_adapters **out);
void flx_adapters_destroy(flx_adapters *adapters);
uint32_t flx_adapters_patterns(const flx_adapters *adapters); /* 2 * n_seqs */
int flx_adapter_cuts(flx_ctx *ctx, flx_adapters *adapters, const uint8_t *plane, uint64_t plane_bytes, const uint64_t *offsets,
                     const int32_t *lengths, const uint32_t *order, uint64_t n_reads, uint32_t *keys);
int flx_adapter_cuts_dev(flx_ctx *ctx, flx_adapters *adapters, const void *d_plane, uint64_t plane_bytes, const void *d_offsets,
                         const void *d_lengths, const void *d_order, uint64_t n_reads, uint32_t *d_keys);
int flx_score_batch_adapters(flx_ctx *ctx, flx_adapters *adapters, const uint8_t *plane, const uint8_t *seq_plane, uint64_t plane_bytes,
                             const uint64_t *offsets, const int32_t *lengths, const uint32_t *order, uint64_t n_reads,
                             const flx_params *params, flx_scores *out);
int flx_score_batch_adapters_dev(flx_ctx *ctx, flx_adapters *adapters, const void *d_plane, const void *d_seq_plane, uint64_t plane_bytes,
                                 const void *d_offsets, const void *d_lengths, const void *d_order, uint64_t n_reads,
                                 const flx_params *params, flx_scores *out_dev);
/* Adapters INSIDE the reads (chimeras; added under version 4).  The same patterns over the whole read, positions 1..L:
 *   hit ends   pattern p of m bases may carry k2 = m * E2 / 100 edits, E2 = split_errors_percent, 0..40; with the recurrence above
 *              d_p(j) = D[m][j], and j is a hit end of p iff d_p(j) <= k2.
 *   marks      every hit end (p, j) marks the bases [max(0, j - m), j); B is the union of all marks.
 *   children   [s, e) is what the ends rule leaves.  No end hit and B empty: no children, first = 0, last = L.  Otherwise the
 *              children are the maximal runs of bases of [s, e) outside B, ascending; first is the first child's start, last the
 *              last child's end.  No base left: no children, first = last = -1 and passed = 0.
 * flx_adapters_set_split: 0..40 turns the middle search on for that object, -1 off (the state after flx_adapters_create); anything
 * else is FLX_ERR_INVALID.  flx_adapters_split: the value set, -1 while off.  flx_score_batch_adapters(_dev) and a pipeline with
 * flx_pipeline_set_adapters follow the object: with the search on a read may have any number of children.
 * flx_adapter_marks(_dev): B as a bitmap over the sequence plane, bit (offsets[i] + b) of it for base b of read i, bit x in
 * 32-bit word x / 32 at x % 32; marks has (plane_bytes + 31) / 32 words, every one written.  Arguments and checks as for
 * flx_adapter_cuts; FLX_ERR_INVALID on an object with the search off.  Timed as "flx_adapter_marks". */
int flx_adapters_set_split(flx_adapters *adapters, int split_errors_percent);
int flx_adapters_split(const flx_adapters *adapters);
/* Adapters that the read begins or ends INSIDE (added under version 4).  The ends rule above charges one edit for every adapter base
 * the read lacks; with an overhang O > 0 every (text, pattern) pair gets a second, anchored walk:
 *   allowance  per pattern of m bases O_p = min(O, m - 12) (12 pattern bases always remain) and k'_p = (m - O_p) * E / 100: the
 *              allowance of the shortest truncated pattern, used for every truncation.  O_p = 0 (m = 12): no second walk.
 *   walk       the same texts and the same recurrence with other borders: D[i][0] = max(0, i - O_p), the first O_p pattern bases may
 *              be missing at no cost; D[0][j] = j, the occurrence begins at the read's edge.  d'(j) = D[m][j], 1 <= j <= n; dmin'
 *              its minimum, jbest' the largest j with d'(j) = dmin'; a hit iff n >= 1 and dmin' <= k'_p.  (d'(j) >= j - m: no j
 *              above m + k'_p can be a hit.)  At the tail the reversed pattern's first bases are the adapter's last: there the
 *              overhang frees the END of the adapter.
 *   keys       per read end, max over every hitting walk, free or anchored, of every pattern of (jbest << 8) | pattern: the key
 *              with an overhang is never below the key without.  cut = key >> 8 and everything behind the keys are unchanged.
 * flx_adapters_set_overhang: O from 0 to 52 (64 - 12); 0, the state after flx_adapters_create, is the ends rule alone in every byte
 * and every launch; anything else is FLX_ERR_INVALID.  A device that already holds the object's patterns gets them again with the
 * next call there.  flx_adapters_overhang: the value set.  flx_adapter_cuts(_dev), flx_score_batch_adapters(_dev) and a pipeline
 * with flx_pipeline_set_adapters follow the object; flx_adapter_marks(_dev) do not depend on it. */
int flx_adapters_set_overhang(flx_adapters *adapters, int overhang);
int flx_adapters_overhang(const flx_adapters *adapters);
int flx_adapter_marks(flx_ctx *ctx, flx_adapters *adapters, const uint8_t *plane, uint64_t plane_bytes, const uint64_t *offsets,
                      const int32_t *lengths, const uint32_t *order, uint64_t n_reads, uint32_t *marks);
int flx_adapter_marks_dev(flx_ctx *ctx, flx_adapters *adapters, const void *d_plane, uint64_t plane_bytes, const void *d_offsets,
                          const void *d_lengths, const void *d_order, uint64_t n_reads, uint32_t *d_marks);

/* ------------------------------------------------------------------------------------------
 * quality trimming of the read ends (added under version 4; the reference has no counterpart: its users run seqtk trimfq, cutadapt
 * -q or chopper --trim-approach over the file first).  Phred mode; the plane holds QUALITY strings.  Defined on integers, on the
 * scale and the table of --split_window_q:
 *   weight     w(b) = (int64)E[b] - (int64)t for quality byte b, E = flx_qsplit_table, 0 <= t < 2^32 (for a quality Q on the 0-100
 *              scale t = flx_qsplit_threshold(Q)): positive for a base worse than the threshold, zero for one exactly on it
 *   head cut   h = the SMALLEST j, 0 <= j <= L, at which P(j) = sum of w(q[i]) for i < j takes its maximum (P(0) = 0: no positive
 *              prefix sum, no cut; ties keep more of the read)
 *   tail cut   c = the smallest c at which S(c) = sum of w(q[L - 1 - i]) for i < c takes its maximum
 * Both cuts are taken over the WHOLE read and independently of each other; |w| < 2^32 and L < 2^31 keep every sum inside int64.
 *   children   the rule of the adapter ends with s = h and e = L - c: both cuts 0: the read goes on as itself (no child, first 0,
 *              last L); s < e: one child [s, e); s >= e: no child, first = last = -1, passed = 0.  A child's scores are the bits
 *              flx_score_batch gives its quality substring, with its own hard cut-offs.
 * flx_endtrim_cuts(_dev): cuts[2 i] = h and cuts[2 i + 1] = c of read i in input order (`order`, NULL or a permutation, only says
 * in which order the reads are processed); a length <= 0 gives 0, 0; every entry is written, none accumulated.  FLX_ERR_INVALID
 * for t >= 2^32.  The work item is a span of flx_endtrim_span() quality bytes of one read (host only: tests place lengths on its
 * edges), the spans of a read are combined in order by a second small kernel.  Timed as "flx_endtrim".
 * flx_score_batch_endtrim(_dev): flx_score_batch_adapters(_dev) with the cuts in the place of the adapters' — the same argument
 * checks, FLX_ERR_CAPACITY with the number of children in out->n_children, params->trim and params->split_set must be 0 — and no
 * sequence plane.
 * ---------------------------------------------------------------------------------------- */
uint32_t flx_endtrim_span(void);
int flx_endtrim_cuts(flx_ctx *ctx, const uint8_t *plane, uint64_t plane_bytes, const uint64_t *offsets, const int32_t *lengths,
                     const uint32_t *order, uint64_t n_reads, uint64_t t, uint32_t *cuts);
int flx_endtrim_cuts_dev(flx_ctx *ctx, const void *d_plane, uint64_t plane_bytes, const void *d_offsets, const void *d_lengths,
                         const void *d_order, uint64_t n_reads, uint64_t t, uint32_t *d_cuts);
int flx_score_batch_endtrim(flx_ctx *ctx, const uint8_t *plane, uint64_t plane_bytes, const uint64_t *offsets, const int32_t *lengths,
                            const uint32_t *order, uint64_t n_reads, const flx_params *params, uint64_t t, flx_scores *out);
int flx_score_batch_endtrim_dev(flx_ctx *ctx, const void *d_plane, uint64_t plane_bytes, const void *d_offsets, const void *d_lengths,
                                const void *d_order, uint64_t n_reads, const flx_params *params, uint64_t t, flx_scores *out);

/* ------------------------------------------------------------------------------------------
 * between seam 2 and seam 3 — the reads2 gather     (replaces src/main.cpp:138-147)
 *
 * reads2 = file order with every trimmed / split parent replaced IN PLACE by its children.  Gathers what the global
 * stage reads (mean quality, window quality, length, pass flag) from the per-read and per-child outputs of
 * flx_score_batch* into reads2 order: entry j is either read parent2[j] itself (child2[j] == -1) or its child number
 * child2[j] (index into the child arrays; length = end - start of its range, src/read.cpp:131-137).  Without children
 * (Phred mode, or no --trim / --split: scores->child_offsets NULL or n_children 0) reads2 is the reads themselves.
 * `capacity` = room in the output arrays (n_reads + n_children always suffices); *n2 = number of entries
 * (FLX_ERR_CAPACITY: *n2 is the capacity needed).  parent2 (uint32) and child2 (int64) may be NULL.
 * _dev: every pointer (also those inside `scores`) is a device pointer; one scan + one scatter kernel on the
 * context's stream.
 * ---------------------------------------------------------------------------------------- */
int flx_reads2_gather_dev(flx_ctx *ctx, uint64_t n_reads, const void *d_lengths, const flx_scores *scores_dev,
                          uint64_t capacity, void *d_mean_q2, void *d_window_q2, void *d_length2, void *d_passed2,
                          void *d_parent2, void *d_child2, uint64_t *n2);
int flx_reads2_gather(flx_ctx *ctx, uint64_t n_reads, const int32_t *lengths, const flx_scores *scores, uint64_t capacity,
                      double *mean_q2, double *window_q2, int32_t *length2, uint8_t *passed2, uint32_t *parent2,
                      int64_t *child2, uint64_t *n2);

/* ------------------------------------------------------------------------------------------
 * seam 3 — global rank + cut     (replaces src/main.cpp:169-261 + Read::set_final_score,
 *                                 src/read.cpp:249-267)
 *
 * Arrays are in "reads2" order: file order with each trimmed/split parent replaced in place by
 * its children (src/main.cpp:138-147).  `passed` is in/out: on return it holds the final pass
 * flags after the --target_bases / --keep_percent cut.  total_bases counts ORIGINAL read lengths
 * (src/main.cpp:89).  final_score (optional) receives the device-computed scores (the reference
 * prints them only under --verbose, 2 decimals); the pass set itself is exact (see DESIGN.md,
 * "boundary audit").
 * ---------------------------------------------------------------------------------------- */
enum flx_cut_outcome {
    FLX_CUT_NONE = 0,          /* neither --target_bases nor --keep_percent given             */
    FLX_CUT_NOT_ENOUGH = 1,    /* "not enough reads to reach target"          main.cpp:239-240 */
    FLX_CUT_ALREADY_BELOW = 2, /* "reads already fall below target after filtering"   242-243 */
    FLX_CUT_SORTED = 3         /* sorted and cut; kept_bases is "keeping N bp"        247-258 */
};

typedef struct flx_cut_report {
    int64_t target_bases;
    int64_t kept_bases;
    int32_t outcome;
    int32_t exact_fallback; /* 1 if a tie group straddled the cut and the host std::sort path decided */
    double mean_quality, stdev_quality, min_z, max_z; /* main.cpp:170-196 */
    uint64_t audited;       /* reads whose score was re-derived with the host libm at the boundary */
} flx_cut_report;

int flx_rank_and_cut(flx_ctx *ctx, uint64_t n, const double *mean_q, const double *window_q, const int32_t *length,
                     uint8_t *passed, double length_weight, double mean_q_weight, double window_q_weight,
                     int target_bases_set, int64_t target_bases, int keep_percent_set, double keep_percent,
                     int64_t total_bases, double *final_score, flx_cut_report *report);

int flx_rank_and_cut_dev(flx_ctx *ctx, uint64_t n, const void *d_mean_q, const void *d_window_q,
                         const void *d_length, void *d_passed, double length_weight, double mean_q_weight,
                         double window_q_weight, int target_bases_set, int64_t target_bases, int keep_percent_set,
                         double keep_percent, int64_t total_bases, void *d_final_score, flx_cut_report *report);

/* The same stage with the reads2 entries sharded over `world` ranks (one process per GPU).  The
 * statistics of src/main.cpp:170-196 are order-dependent folds over ALL mean qualities, so d_mean_q_all holds every
 * rank's mean qualities in global reads2 order (the one array that has to be all-gathered: 8 bytes per entry).
 * Everything else stays local: d_window_q / d_length / d_passed / d_final_score describe this rank's entries
 * [first, first + n_local) only.  The cut (src/main.cpp:247-257) is a weighted selection: per key byte a 256-bin
 * histogram of summed read lengths, whose global value is the SUM over ranks — the only exchange the selection
 * needs.  `reduce(user, buf, count)` must replace buf[0..count) (host memory) by its element-wise sum over all
 * ranks and return 0; it is called the same number of times with the same counts on every rank (about a dozen
 * calls of <= 2 KB + one of 40 bytes per boundary-audit candidate).  NULL is allowed when world == 1.
 * Returns FLX_OK with this rank's final pass flags in d_passed (report fields are global), or
 * FLX_NEED_REPLICATED — on every rank alike, before anything was modified — when the exact outcome needs the
 * reference's own std::sort over all records (NaN scores, equal scores straddling the cut, or FLX_RANK_SORT=1):
 * gather the records and call flx_rank_and_cut_dev. */
typedef int (*flx_allreduce_u64_fn)(void *user, uint64_t *buf, uint64_t count);

int flx_rank_and_cut_sharded_dev(flx_ctx *ctx, uint64_t n_total, const void *d_mean_q_all, uint64_t first,
                                 uint64_t n_local, const void *d_window_q, const void *d_length, void *d_passed,
                                 double length_weight, double mean_q_weight, double window_q_weight,
                                 int target_bases_set, int64_t target_bases, int keep_percent_set, double keep_percent,
                                 int64_t total_bases, void *d_final_score, int rank, int world,
                                 flx_allreduce_u64_fn reduce, void *user, flx_cut_report *report);

/* ------------------------------------------------------------------------------------------
 * seam 2, streaming — replaces the pass-1 loop of src/main.cpp:70-127 for inputs larger than memory
 *
 * The caller parses its input chunk by chunk.  For every chunk:
 *     flx_pipeline_next_buffer -> a PINNED staging buffer of `capacity_bytes` (blocks while both slots are in flight)
 *     pack the chunk's reads into it (flx_plane_layout gives offsets and the byte count; Phred mode: quality strings,
 *     k-mer mode: sequences — as for flx_score_batch)
 *     flx_pipeline_submit      -> starts the H2D copy and returns; a worker thread scores the chunk when it has landed
 * so chunk k is copied and scored on the GPU while the host packs chunk k+1 (two slots).  flx_pipeline_finish waits for
 * everything and returns the per-read results of ALL submitted reads in submission order as host arrays owned by the
 * pipeline (children in one global CSR); only these scalars survive between the chunks, like the reference, which keeps
 * one Read object per record and drops the record's text.  The context must not be used for anything else between
 * create and finish (its stream belongs to the worker).
 * ---------------------------------------------------------------------------------------- */
typedef struct flx_pipeline flx_pipeline;
int flx_pipeline_create(flx_ctx *ctx, const flx_kmerset *set /* NULL or empty: Phred mode */, const flx_params *params,
                        uint64_t chunk_plane_bytes, uint64_t chunk_reads, flx_pipeline **out);
/* --split_window_q for a Phred-mode pipeline (added under version 4): every chunk then goes through flx_score_batch_qsplit_dev and
 * flx_pipeline_finish returns the children in its global CSR.  Before the first submit; FLX_ERR_STATE on a pipeline with a non-empty
 * set or after a submit, FLX_ERR_INVALID unless 0 < q < 100. */
int flx_pipeline_set_qsplit(flx_pipeline *p, double q);
/* --exclude for a pipeline (added under version 4): every chunk also goes through flx_screen_hits_dev against `exclude_set` (filled
 * with flx_screen_set_add, finalized, not empty: FLX_ERR_STATE otherwise), on the context's stream behind the scoring; a read with
 * windows > 0 and (hits << 32) >= t * windows, t = flx_screen_threshold(percent), is treated like a read that fails a hard cut-off: its
 * pass flag and those of all its children are cleared on the device before the results come back.  It stays an entry.  Before the
 * first flx_pipeline_next_buffer; FLX_ERR_STATE afterwards, FLX_ERR_INVALID unless 0 < percent <= 100.  In a k-mer-mode pipeline the
 * one plane (sequences) serves the scoring and the screen.  In a Phred-mode pipeline a chunk then carries TWO planes with the same
 * offsets: the qualities at [0, plane_bytes) and the sequences at [plane_bytes, 2 plane_bytes) of the staging buffer; plane_bytes,
 * chunk_plane_bytes, capacity_bytes and flx_pipeline_reserve keep meaning ONE plane, the buffer has room for two.
 * flx_pipeline_screen: the hits and the excluded flags (1 / 0) of all reads in submission order, host arrays owned by the pipeline,
 * after flx_pipeline_finish. */
int flx_pipeline_set_screen(flx_pipeline *p, const flx_kmerset *exclude_set, double percent);
int flx_pipeline_screen(flx_pipeline *p, const uint32_t **hits, const uint8_t **excluded);
/* --exclude with --exclude_k for a pipeline: flx_pipeline_set_screen with a flx_screenset — the same state rules, the same two planes
 * in Phred mode, windows = max(0, L - K + 1) in the decision, and flx_pipeline_screen afterwards.  A pipeline takes one of the two
 * calls: the other one is then FLX_ERR_STATE. */
int flx_pipeline_set_screenset(flx_pipeline *p, const flx_screenset *exclude_set, double percent);
/* --trim_adapters for a Phred-mode pipeline (added under version 4): every chunk then goes through flx_score_batch_adapters_dev.
 * The chunk carries the second plane exactly as flx_pipeline_set_screen arranged it (qualities, then the sequences at the same
 * offsets; with both a screen and adapters there is still ONE sequence plane).  The screen keeps looking at the whole parent; an
 * excluded parent's child fails.  Before the first flx_pipeline_next_buffer; FLX_ERR_STATE afterwards, on a pipeline with a non-empty
 * set, or together with flx_pipeline_set_qsplit (in either order).
 * flx_pipeline_adapters: the keys (head, tail) of all reads in submission order, a host array of 2 n entries owned by the pipeline,
 * valid after flx_pipeline_finish until the pipeline is destroyed. */
int flx_pipeline_set_adapters(flx_pipeline *p, flx_adapters *adapters);
int flx_pipeline_adapters(flx_pipeline *p, const uint32_t **keys);
/* --max_low_complexity for a pipeline (added under version 4): every chunk also goes through flx_complexity_bad_dev, on the
 * context's stream behind the scoring and behind the screen; a flagged read (above) is treated exactly like an excluded one: its pass
 * flag and those of all its children are cleared on the device, and it stays an entry.  The state rules of flx_pipeline_set_screen:
 * before the first flx_pipeline_next_buffer, FLX_ERR_STATE afterwards; FLX_ERR_INVALID unless 0 < percent <= 100 and 10 <= score_t
 * <= 300.  In a Phred-mode pipeline the chunk carries the two planes exactly as a screen or adapters arrange them (with those as
 * well there is still ONE sequence plane).  A screen and this filter may both be set; a read flagged by both shows in both.
 * flx_pipeline_complexity: the bad windows and the flags (1 / 0) of all reads in submission order, host arrays owned by the
 * pipeline, after flx_pipeline_finish. */
int flx_pipeline_set_complexity(flx_pipeline *p, double percent, int score_t);
int flx_pipeline_complexity(flx_pipeline *p, const uint32_t **bad, const uint8_t **flagged);
/* --trim_ends_q for a Phred-mode pipeline (added under version 4): every chunk then goes through flx_score_batch_endtrim_dev with
 * t = flx_qsplit_threshold(q); the chunk stays ONE plane of qualities unless a screen or the low-complexity filter adds the sequences.
 * FLX_ERR_INVALID unless 0 < q < 100; FLX_ERR_STATE after the first flx_pipeline_next_buffer / flx_pipeline_submit, on a pipeline
 * with a k-mer set, and together with flx_pipeline_set_qsplit or flx_pipeline_set_adapters (in either order: the producers of
 * children do not compose).
 * flx_pipeline_endtrim: the cuts (head, tail) of all reads in submission order, a host array of 2 n entries owned by the pipeline,
 * after flx_pipeline_finish. */
int flx_pipeline_set_endtrim(flx_pipeline *p, double q);
int flx_pipeline_endtrim(flx_pipeline *p, const uint32_t **cuts);
int flx_pipeline_next_buffer(flx_pipeline *p, uint8_t **plane, uint64_t *capacity_bytes, uint64_t *capacity_reads);
/* Grow both slots to at least this capacity (never shrinks; waits for the chunks in flight first).  For callers that learn
 * the longest read only while streaming.  Not between next_buffer and submit. */
int flx_pipeline_reserve(flx_pipeline *p, uint64_t chunk_plane_bytes, uint64_t chunk_reads);
int flx_pipeline_submit(flx_pipeline *p, uint64_t plane_bytes, const uint64_t *offsets, const int32_t *lengths, uint64_t n_reads);
int flx_pipeline_finish(flx_pipeline *p, flx_scores *all, uint64_t *n_reads);
void flx_pipeline_destroy(flx_pipeline *p);

/* Multi-GPU without a host framework: one process per GPU, each with one context; the library owns the RCCL communicator
 * (loaded with dlopen on first use) and does the exchange of the global stage itself, on device buffers on the context's
 * stream (no host synchronisation inside the 8 selection passes):
 *     rank 0: flx_comm_unique_id(ctx, id) -> hand the 128 bytes to every rank (file, socket, launcher, ...)
 *     all:    flx_comm_init(ctx, id, rank, world)
 *     all:    flx_score_batch_dev(...) on the rank's own reads (contiguous block of file order, sharded by count)
 *     all:    flx_rank_and_cut_comm_dev(...)  = ONE all-gather of the mean qualities over xGMI + the sharded stage above;
 *             the rare NaN / tie cases that need the reference's std::sort over all reads gather the remaining fields and
 *             run the replicated stage internally.  `total_bases` is the GLOBAL sum (flx_comm_sum_u64 helps).
 * Without a communicator flx_rank_and_cut_comm_dev is flx_rank_and_cut_dev.  The reference has no counterpart (single
 * process, src/main.cpp:37-321). */
#define FLX_COMM_ID_BYTES 128
int flx_comm_unique_id(flx_ctx *ctx, void *id_out /* FLX_COMM_ID_BYTES */);
int flx_comm_init(flx_ctx *ctx, const void *id, int rank, int world);
int flx_comm_destroy(flx_ctx *ctx);
int flx_comm_rank(const flx_ctx *ctx);
int flx_comm_world(const flx_ctx *ctx);
int flx_comm_sum_u64(flx_ctx *ctx, uint64_t *host_buf, uint64_t count); /* element-wise sum over all ranks, in place */
/* host-array variant (the arrays are staged through the device, like flx_rank_and_cut) */
int flx_rank_and_cut_comm(flx_ctx *ctx, uint64_t n_local, const double *mean_q, const double *window_q, const int32_t *length,
                          uint8_t *passed, double length_weight, double mean_q_weight, double window_q_weight,
                          int target_bases_set, int64_t target_bases, int keep_percent_set, double keep_percent,
                          int64_t total_bases, double *final_score, flx_cut_report *report);
int flx_rank_and_cut_comm_dev(flx_ctx *ctx, uint64_t n_local, const void *d_mean_q, const void *d_window_q,
                              const void *d_length, void *d_passed, double length_weight, double mean_q_weight,
                              double window_q_weight, int target_bases_set, int64_t target_bases, int keep_percent_set,
                              double keep_percent, int64_t total_bases, void *d_final_score, flx_cut_report *report);

/* ------------------------------------------------------------------------------------------
 * seam 1 — reference 16-mer set   (replaces Kmers, src/kmers.cpp:28-172 + src/bloom_filter.h)
 *
 * Sequences are handed over packed: bases[offsets[i] .. offsets[i]+lengths[i]).  Call order for
 * short reads must be the reference's: all of -1, then all of -2 (src/kmers.cpp:54-55); the
 * ">= 4 copies, or 3 with a Bloom false positive" rule (src/kmers.cpp:142-166) is order
 * dependent only through the Bloom filter, which is restated bit-exactly.
 * After flx_kmerset_finalize the set is immutable.  An empty finalized set selects Phred mode,
 * like Kmers::empty() (src/kmers.h:34, src/read.cpp:35).
 * ---------------------------------------------------------------------------------------- */
int flx_kmerset_create(flx_ctx *ctx, flx_kmerset **out);
void flx_kmerset_destroy(flx_kmerset *set);
int flx_kmerset_add_assembly(flx_kmerset *set, const uint8_t *bases, const uint64_t *offsets,
                             const int64_t *lengths, uint64_t n_seqs);
int flx_kmerset_add_short_reads(flx_kmerset *set, const uint8_t *bases, const uint64_t *offsets,
                                const int64_t *lengths, uint64_t n_seqs);
int flx_kmerset_finalize(flx_kmerset *set);
uint64_t flx_kmerset_size(const flx_kmerset *set);
int flx_kmerset_contains(const flx_kmerset *set, const uint32_t *kmers, uint64_t n, uint8_t *present);

/* ------------------------------------------------------------------------------------------
 * BGZF compression (added under version 4): gzip members of at most 65280 input bytes (member k holds bytes
 * [k*65280, (k+1)*65280) of the input), each with the BC extra field of the SAM/BAM specification §4.1, each compressed
 * on its own by one workgroup (one dynamic-Huffman deflate block, or one stored block when that is not larger).
 * Plain gzip to any gzip reader; FLX_BGZF_EOF appends the 28-byte end-of-file block.  The output is a pure function of
 * (bytes, flags); an input of 0 bytes gives 0 bytes, or just the end-of-file block.
 *   flx_bgzf_bound          the most bytes a call can write: n + 31 per member (+ 28)
 *   flx_bgzf_compress_dev   device to device, on the context's stream (timed as "flx_bgzf"); FLX_ERR_CAPACITY when out_cap
 *                           is below the compressed size (*out_len 0; what was written is no result)
 *   flx_bgzf                host to host with its own streams and pinned slots of slot_bytes (rounded down to a multiple
 *                           of 65280) each: the ONE object of the ABI that may be called from several threads at once;
 *                           concurrent calls take different slots and overlap their copies and kernels.  A call of more
 *                           than slot_bytes runs in slot-sized pieces on one slot (the same bytes as one piece).
 * ---------------------------------------------------------------------------------------- */
#define FLX_BGZF_EOF 1 /* append the 28-byte BGZF end-of-file block */
int flx_bgzf_bound(uint64_t n, int flags, uint64_t *bound);
int flx_bgzf_compress_dev(flx_ctx *ctx, const void *d_in, uint64_t n, int flags, void *d_out, uint64_t out_cap,
                          uint64_t *out_len);
typedef struct flx_bgzf flx_bgzf;
int flx_bgzf_create(flx_ctx *ctx, uint64_t slot_bytes, unsigned slots, flx_bgzf **out);
int flx_bgzf_compress(flx_bgzf *z, const void *in, uint64_t n, int flags, void *out, uint64_t out_cap, uint64_t *out_len);
void flx_bgzf_destroy(flx_bgzf *z);

/* BGZF members inflated on the device (added under version 4): the read side of the compressor.  A member holds at most 64 KiB,
 * carries its size and depends on no other, so members are decoded side by side, one wave each.  The decoder is a complete RFC 1951
 * decoder (stored, fixed and dynamic blocks, any number per member); a member is ok (status word 0) only when its deflate data is
 * valid, ends in the last byte in front of the trailer, gives exactly ISIZE bytes and their CRC-32 is the trailer's.  In doubt it
 * rejects: a caller hands the first bad member to zlib, which has the last word on damaged data.  The bytes of a member that is not
 * ok are unspecified (and inside its own range).
 *   flx_bgzf_index        host only, no device: walks the well-formed BGZF members from byte 0 (magic, CM 8, FEXTRA with a `BC`
 *                         subfield of length 2, BSIZE + 1 within n and no smaller than header + 8, ISIZE <= 65536) up to the
 *                         first that is not, or max_members.  in_off[0..m] and out_off[0..m] are the prefix sums of the members'
 *                         sizes and of their ISIZEs (m + 1 entries each, so room for max_members + 1); *n_members = m.
 *   flx_bgzf_inflate_dev  device to device on the context's stream (timed as "flx_bgzf_inflate"): member k is the bytes
 *                         [d_in_off[k], d_in_off[k+1]) of d_in and its output goes to [d_out_off[k], d_out_off[k+1]) of d_out;
 *                         d_status[k] = 0 for an ok member.  *first_bad = the lowest k with a status other than 0, or n_members;
 *                         it comes back with the call's one small copy.  FLX_OK whenever the call ran: a damaged member is
 *                         data, not an error.  n_members == 0 is a no-op.
 *   flx_bgzf_inflate      host to host through the pinned slots and streams of a flx_bgzf; may be called from several threads at
 *                         once like flx_bgzf_compress.  Offsets as above, relative to `in` and `out`.  Runs in pieces that fit a
 *                         slot both ways and stops behind the piece of the first bad member: the bytes of the members in front
 *                         of *first_bad are in `out`, nothing behind them is promised.
 * ---------------------------------------------------------------------------------------- */
int flx_bgzf_index(const void *in, uint64_t n, uint64_t max_members, uint64_t *in_off, uint64_t *out_off, uint64_t *n_members);
int flx_bgzf_inflate_dev(flx_ctx *ctx, const void *d_in, const uint64_t *d_in_off, const uint64_t *d_out_off, uint64_t n_members,
                         void *d_out, uint32_t *d_status, uint64_t *first_bad);
int flx_bgzf_inflate(flx_bgzf *z, const void *in, const uint64_t *in_off, const uint64_t *out_off, uint64_t n_members, void *out,
                     uint64_t *first_bad);

/* ------------------------------------------------------------------------------------------
 * unaligned BAM to FASTQ text (added under version 4): the layer inside the BGZF container.  Input is INFLATED BAM (SAM/BAM
 * specification 4.2): the header, then records that each start with their block_size.  A record is valid when block_size >= 32,
 * l_read_name >= 1 with a NUL as the name's last byte, l_seq >= 0, 32 + l_read_name + 4 n_cigar_op + (l_seq + 1) / 2 + l_seq <=
 * block_size (in 64 bits) and it lies inside the buffer; CIGAR and tags are skipped, never interpreted.  Its text is
 *   '@' name '\n' SEQ '\n' '+' '\n' QUAL '\n'      (l_read_name + 2 l_seq + 5 bytes; at most twice the record's block_size + 4)
 * with SEQ from "=ACMGRSVTWYHKDBN", QUAL = min(q, 93) + 33, or '"' (quality 1) at every position when the first quality byte is 0xFF
 * (no qualities stored); flag 0x10 gives the reverse complement (IUPAC; '=' and 'N' stay) and the reversed qualities; flags 0x40 /
 * 0x80 do not change the name.  A record with flag 0x100 or 0x800 (secondary, supplementary) or with l_seq == 0 has no text: it is
 * skipped and counted.
 *   flx_bam_index         host only, no device: checks the header and walks the records from the first to the last whole, valid one
 *                         within n bytes, or to max_records.  rec_off[0..m] are the records' offsets (rec_off[0]: the end of the
 *                         header; m + 1 entries, so room for max_records + 1; NULL: count only), *n_records = m and *end_state
 *                         tells why the walk ended (FLX_BAM_*): a rule that the bytes present already break is MALFORMED
 *                         (HEADER inside the header), a buffer that ends before a rule can be checked is TRUNCATED.
 *   flx_bam_to_fastq_dev  device to device on the context's stream (timed as "flx_bam"): record k is the bytes [d_rec_off[k],
 *                         d_rec_off[k+1]) of d_bam[0, n).  d_out_off[0..n_records] (device, u64) gets the text offsets: a skipped
 *                         record has d_out_off[k+1] == d_out_off[k]; *out_len the text length, *n_skipped the skipped records.
 *                         FLX_ERR_CAPACITY when out_cap is below the text length (*out_len = the length needed; nothing is
 *                         written).  A record the device finds invalid is data, not an error: *first_bad = the lowest such k (else
 *                         n_records), it counts as no text, and the text is then no result.  n_records == 0 is a no-op.
 *   flx_bam_to_fastq      host to host through two pinned staging slots with a stream each, in pieces of whole records of at most
 *                         piece_bytes of BAM (0: 32 MiB; the staging grows to the largest record): copy-in, kernels and copy-out
 *                         of consecutive pieces overlap.  out_off (host, n_records + 1 entries) may be NULL.  Stops in front of
 *                         *first_bad: the text of the records before it is in out.  FLX_ERR_CAPACITY as above.
 * ---------------------------------------------------------------------------------------- */
#define FLX_BAM_END 0       /* the last record ends where the data ends                         */
#define FLX_BAM_TRUNCATED 1 /* the data ends inside the header or inside record *n_records      */
#define FLX_BAM_MALFORMED 2 /* record *n_records breaks a rule                                  */
#define FLX_BAM_HEADER 3    /* the header does: no magic, a negative length                     */
#define FLX_BAM_MORE 4      /* max_records were taken and data is left                          */
int flx_bam_index(const void *bam, uint64_t n, uint64_t max_records, uint64_t *rec_off, uint64_t *n_records, int *end_state);
int flx_bam_to_fastq_dev(flx_ctx *ctx, const void *d_bam, uint64_t n, const uint64_t *d_rec_off, uint64_t n_records, void *d_out,
                         uint64_t out_cap, uint64_t *d_out_off, uint64_t *out_len, uint64_t *n_skipped, uint64_t *first_bad);
int flx_bam_to_fastq(flx_ctx *ctx, const void *bam, uint64_t n, const uint64_t *rec_off, uint64_t n_records, uint64_t piece_bytes,
                     void *out, uint64_t out_cap, uint64_t *out_off, uint64_t *out_len, uint64_t *n_skipped, uint64_t *first_bad);

/* ------------------------------------------------------------------------------------------
 * FASTQ / FASTA text to unaligned BAM (added under version 4): the write side of the functions above.  Input is STRICT record text:
 * record k is the bytes [rec_off[k], rec_off[k+1]) and has the form
 *   '@' HEADER '\n' SEQ '\n' '+' '\n' QUAL '\n'    (FASTQ, |SEQ| == |QUAL| == L)      or      '>' HEADER '\n' SEQ '\n'    (FASTA)
 * Only the header line is scanned (to its first '\n'); L follows from the record's length and the bytes at the derived positions
 * must be '\n', '+', '\n', '\n'.  The name is the header up to its first blank or tab; the rest of the line (the comment) is NOT
 * stored.  A record is valid when it has that shape, the name has 1..254 bytes, L <= 2^31 - 1 and every QUAL byte is in 33..126.
 * Its BAM record: refID -1, pos -1, mapq 0, bin 4680, no CIGAR, flag 4, next_refID -1, next_pos -1, tlen 0, the name, the bases
 * packed by "=ACMGRSVTWYHKDBN" (upper-cased; any other byte is 'N'; a zero low nibble behind an odd L), the qualities c - 33 (0xFF
 * at every position for a FASTA record), no tags: 37 + name + (L + 1) / 2 + L bytes.
 *   flx_bam_header            host only: the header of a file written from text ("BAM\1", l_text, "@HD\tVN:1.6\tSO:unknown\n", n_ref 0);
 *                             *out_len = its size; out == NULL: the size only; FLX_ERR_CAPACITY when out_cap is below it.
 *   flx_bam_from_fastq_bound  the most bytes the records of n_text bytes of text in n_records records can take:
 *                             n_text + n_text / 2 + 34 n_records (a FASTA record of L bases grows by 34 + ceil(L/2) at most, a FASTQ
 *                             record by 31 at most).
 *   flx_bam_from_fastq_dev    device to device on the context's stream (timed as "flx_bam_encode"): d_out_off[0..n_records] (device,
 *                             u64) gets the records' offsets in d_out, *out_len the BAM length.  FLX_ERR_CAPACITY when out_cap is
 *                             below it (*out_len = the length needed; nothing is written).  An invalid record is data, not an
 *                             error: *first_bad = the lowest such k (else n_records), and the output is then no result.  Offsets
 *                             that leave [0, n) or run backwards make their records invalid.  n_records == 0 is a no-op.
 *   flx_bgzf_bam_from_fastq   host to host through ONE slot of a flx_bgzf: the text is uploaded, encoded, the encoded bytes are
 *                             compressed by the kernels of flx_bgzf_compress_dev and the compressed bytes come back; the uncompressed
 *                             BAM never crosses the link.  May be called from several threads at once like flx_bgzf_compress.
 *                             rec_off is relative to `text` (rec_off[0] .. rec_off[n_records] <= n).  Text beyond the slot goes
 *                             through in pieces of whole records and the slot's buffers grow to the largest record.  The
 *                             DECOMPRESSED bytes are a pure function of the text; where the members are cut depends on the pieces.
 *                             FLX_BGZF_EOF as for the compressor.  out_cap of flx_bgzf_bound(flx_bam_from_fastq_bound(..)) + 31
 *                             n_records always suffices (a piece ends with a member of its own); FLX_ERR_CAPACITY below what is
 *                             needed.  With an invalid record: FLX_OK, *first_bad = its number, *out_len = 0, `out` is no result.
 * ---------------------------------------------------------------------------------------- */
int flx_bam_header(void *out, uint64_t out_cap, uint64_t *out_len);
int flx_bam_from_fastq_bound(uint64_t n_text, uint64_t n_records, uint64_t *bound);
int flx_bam_from_fastq_dev(flx_ctx *ctx, const void *d_text, uint64_t n, const uint64_t *d_rec_off, uint64_t n_records, void *d_out,
                           uint64_t out_cap, uint64_t *d_out_off, uint64_t *out_len, uint64_t *first_bad);
int flx_bgzf_bam_from_fastq(flx_bgzf *z, const void *text, uint64_t n, const uint64_t *rec_off, uint64_t n_records, int flags, void *out,
                            uint64_t out_cap, uint64_t *out_len, uint64_t *first_bad);

/* ------------------------------------------------------------------------------------------
 * read summary (added under version 4): what a set of reads looks like — entries, bases, shortest, longest, median, N10..N90
 * and the histograms of length, mean quality and window quality — from the per-read arrays of seam 2 / the reads2 gather and
 * the pass flags of seam 3.  The reference has no counterpart: its users run a statistics tool over the input and again over
 * the output.  Every field is an integer and every definition is exact, so N ranks give the bits of one rank.
 *   which entries count   all when mask is NULL, else those with mask[i] != 0; lengths must not be negative (FLX_ERR_INVALID)
 *   length bins           bin 0 holds lengths 0 and 1, bin b holds 2^b <= L < 2^(b+1)
 *   quality bins          on the Phred scale: edges[k] = 100 (1 - 10^(-k/10)), k = 0..50, computed once with the host's pow
 *                         (flx_summary_q_edges returns the very doubles the kernel bins with); bin k in 0..49 holds
 *                         edges[k] <= q < edges[k+1], bin 50 q >= edges[50] (100.0 included), bin 51 NaN and q < 0.  A NULL
 *                         quality array leaves its two histograms zero.  *_count = entries, *_bases = sum of their lengths.
 *   Nx                    order the counted entries by descending length; Nx is the length of the first entry at which
 *                         100 * cum >= x * bases, cum = the sum of the lengths up to and including that entry (the product
 *                         is carried in 128 bits); 0 when bases == 0.  nx[0] = N10 ... nx[4] = N50 ... nx[8] = N90.
 *   median_length         entry (n - 1) / 2 of the ascending order (the lower median)
 *   global                != 0 on a context with a communicator (flx_comm_init): the call is COLLECTIVE — every rank calls it
 *                         (a rank with n == 0 too), every count and histogram is summed over the ranks (the exchange of
 *                         flx_comm_sum_u64) and every rank returns the same struct, that of all entries of all ranks.
 *                         Without a communicator `global` is ignored.
 * One streaming pass over the arrays for the histograms and four over length and mask for the ten order statistics (radix
 * selection, 8 bits per pass); five small device-to-host copies (<= 40 KiB) per call.  The timing bracket "flx_summary" spans the
 * whole call on the stream: kernels, copies, the host's work between the passes and, when collective, the exchanges.
 * In C the struct is named with its tag, `struct flx_summary`: the plain name is the function's.
 * ---------------------------------------------------------------------------------------- */
#define FLX_SUMMARY_LEN_BINS 32
#define FLX_SUMMARY_Q_BINS 52
struct flx_summary {
    uint64_t n, bases;               /* entries counted, sum of their lengths              */
    int32_t min_length, max_length;  /* 0, 0 when n == 0                                   */
    int32_t median_length, _pad0;    /* 0 when n == 0                                      */
    int32_t nx[9];                   /* N10, N20, ... N90                                  */
    int32_t _pad1;
    uint64_t len_count[FLX_SUMMARY_LEN_BINS], len_bases[FLX_SUMMARY_LEN_BINS];
    uint64_t mean_q_count[FLX_SUMMARY_Q_BINS], mean_q_bases[FLX_SUMMARY_Q_BINS];
    uint64_t window_q_count[FLX_SUMMARY_Q_BINS], window_q_bases[FLX_SUMMARY_Q_BINS];
};
int flx_summary_q_edges(double edges[51]);
int flx_summary_dev(flx_ctx *ctx, uint64_t n, const void *d_length /* int32 */, const void *d_mean_q /* f64 or NULL */,
                    const void *d_window_q /* f64 or NULL */, const void *d_mask /* u8, or NULL = all */, int global,
                    struct flx_summary *out /* host */);
/* host arrays, staged through the device like flx_rank_and_cut */
int flx_summary(flx_ctx *ctx, uint64_t n, const int32_t *length, const double *mean_q, const double *window_q,
                const uint8_t *mask, int global, struct flx_summary *out);

/* ------------------------------------------------------------------------------------------
 * bench / test support: deterministic synthetic Phred planes generated directly in HBM
 * (same integer hash as filtlong_amd/synth.py and oracle/synth.h).
 * d_read_ids[i] is the global index of read i in the synthetic population.
 * ---------------------------------------------------------------------------------------- */
int flx_synth_qual_dev(flx_ctx *ctx, uint64_t seed, void *d_plane, uint64_t plane_bytes, const void *d_offsets,
                       const void *d_lengths, const void *d_read_ids, uint64_t n_reads);
/* the same with a quality profile: 0 = the SURVEY §8(d) definition (what flx_synth_qual_dev writes), 1 = "wide": per-read
 * centre Q3..Q44, per-base jitter +-10, q <= 50 (a realistic spread; bench.py's second Phred line) */
int flx_synth_qual_profile_dev(flx_ctx *ctx, uint64_t seed, int profile, void *d_plane, uint64_t plane_bytes,
                               const void *d_offsets, const void *d_lengths, const void *d_read_ids, uint64_t n_reads);

/* k-mer configurations: reads drawn from a device-resident reference genome (d_ref, ASCII ACGT) with per-read
 * substitution rates and junk blocks. */
int flx_synth_seq_dev(flx_ctx *ctx, uint64_t seed, void *d_plane, uint64_t plane_bytes, const void *d_offsets,
                      const void *d_lengths, const void *d_read_ids, uint64_t n_reads, const void *d_ref,
                      uint64_t ref_len);
/* the same with a profile: 0 = the SURVEY §8(d) definition (what flx_synth_seq_dev writes: substitutions only), 1 = "indels": the same
 * per-read error rate, a third of the errors insertions and a third deletions of 1-3 bases, 2 = "unrelated": 30 % of the reads are
 * random bases with no relation to the reference (oracle/synth.h: flx_synth_seq_read; bench.py's extras.c3_indels / .c3_unrelated) */
int flx_synth_seq_profile_dev(flx_ctx *ctx, uint64_t seed, int profile, void *d_plane, uint64_t plane_bytes, const void *d_offsets,
                              const void *d_lengths, const void *d_read_ids, uint64_t n_reads, const void *d_ref,
                              uint64_t ref_len);

#ifdef __cplusplus
}
#endif
#endif /* FILTLONG_HIP_H */
