"""--exclude with --exclude_k 24 through the whole command line, against tests/_screen_k_model.py: stdout is the run without the flag
minus exactly the reads the model excludes (and the children of those) by every road — plain, streamed gzip and BAM input, --gzip,
--bam, --gpus 2, -a mode, --split_window_q — with the reference handed over in batches of a few hundred bytes; the stderr lines, the
--verbose line, --report's fourth summary and a --keep_percent cut are the model's; --exclude_k 16 is the run without the flag, byte
for byte; the too-many refusal at K = 17.  Every test first makes sure that the model excludes some reads and keeps others."""
import gzip
import json
import re
import sys

import numpy as np
import pytest

import _bam
import _bgzf
import _oracle
import _qsplit_model as qmodel
import _screen_k_model as model
from test_exclude_cli_gpu import fastq_bytes, records, run, shim_env, without

pytestmark = pytest.mark.gpu
K = 24
SMALL_BATCHES = {"FLX_CLI_REF_BATCH_BYTES": "300"}
gen_bam = sys.modules["gen_bam"]  # (tools/gen_bam.py, put on the path by test_exclude_cli_gpu)


@pytest.fixture(scope="module")
def made(tmp_path_factory):
    """60 reads: 20 from a 5 kbp contaminant (both strands, 0 to 5 % substitutions; read 0 is a chimera, half contaminant), 40 from a
    60 kbp genome the contaminant has nothing to do with; some with a junk stretch in their qualities.  The contaminant's FASTA has 25
    records of 200 bases (no window spans two of them), one with a run of N"""
    d = tmp_path_factory.mktemp("exclude_k_cli")
    rng = np.random.default_rng(919)
    xref, gref = model.random_seq(rng, 5000), model.random_seq(rng, 60000)
    reads = []
    for i in range(60):
        n = int(rng.integers(600, 4000))
        if i == 0:
            seq = model.draw(rng, gref, 1500, 0.02) + model.draw(rng, xref, 1500, 0.02)
        elif i % 3 == 0:
            seq = model.draw(rng, xref, n, (0.0, 0.02, 0.05)[i % 9 // 3])
        else:
            seq = model.draw(rng, gref, n, 0.02)
        st = [(len(seq) // 2, len(seq) // 2 + 350)] if i % 4 == 1 or i == 6 else []
        reads.append((b"read_%d" % i, seq, qmodel.junk_read(rng, len(seq), st, good=(25, 40), junk=(0, 3))))
    pieces = [xref[a:a + 200] for a in range(0, 5000, 200)]
    pieces[7] = pieces[7][:90] + b"N" * 20 + pieces[7][110:]
    x_fa = b"".join(b">piece %d\n" % i + p + b"\n" for i, p in enumerate(pieces))
    (d / "x.fa").write_bytes(x_fa)
    (d / "x.fa.gz").write_bytes(gzip.compress(x_fa))
    (d / "g.fa").write_bytes(b">g\n" + gref + b"\n")
    (d / "made.fastq").write_bytes(fastq_bytes(reads))
    (d / "made.fastq.gz").write_bytes(gzip.compress(fastq_bytes(reads)))
    (d / "made.bam").write_bytes(gen_bam.bgzf(gen_bam.fastq_to_bam(fastq_bytes(reads))))
    x = model.build_set(pieces, K)
    hits = [int(h) for h in model.hits_many(x, [s for _, s, _ in reads], K)]
    out = {"dir": d, "reads": reads, "x": str(d / "x.fa"), "xgz": str(d / "x.fa.gz"), "g": str(d / "g.fa"), "fastq": str(d / "made.fastq"),
           "gz": str(d / "made.fastq.gz"), "bam": str(d / "made.bam"), "hits": hits, "keys": len(x), "pieces": pieces}
    for pct in (10.0, 60.0):
        out[pct] = [model.excluded(h, len(s), pct, K) for h, (_, s, _) in zip(hits, reads)]
    assert sum(out[10.0]) == 20 and out[10.0][0] and not out[60.0][0] and 0 < sum(out[60.0]) < 20
    return out


def names(made, pct=10.0):
    got = {n for (n, _, _), e in zip(made["reads"], made[pct]) if e}
    assert 0 < len(got) < len(made["reads"])  # the model excludes at least one read and keeps at least one
    return got


def excluded_line(made, pct=10.0):
    return b"  excluded by reference: %d reads (%d bp)\n" % (sum(made[pct]), sum(len(s) for (_, s, _), e in zip(made["reads"], made[pct]) if e))


FLAG = ["--exclude_k", str(K)]


def test_stdout_is_the_run_without_the_flag_minus_the_excluded(made):
    rc, plain, err0 = run(["--min_length", "1", made["fastq"]])
    assert rc == 0 and plain == fastq_bytes(made["reads"]) and b"excluded" not in err0
    rc, out, err = run(["--exclude", made["x"], "--min_length", "1", made["fastq"]] + FLAG, SMALL_BATCHES)
    assert rc == 0 and b"Error" not in err, err[-2000:]
    assert out == without(plain, names(made)) and len(records(out)) == 40
    assert excluded_line(made) in err and err.index(excluded_line(made)) > err.index(b"60 reads")
    # the lines of the set: the header with K, the file, its progress line, the sequences and the canonical keys
    total = sum(len(p) for p in made["pieces"])
    want = (b"Hashing 24-mers to exclude\n  " + made["x"].encode() + b"\n\r  " + made["x"].encode() + b" (%d bp)\n" % total
            + b"  25 sequences, %d canonical 24-mers\n\n" % made["keys"])
    assert want in err and b"16-mers" not in err
    # one batch gives the same set; the flag alone is a threshold; a gzip FASTA is read like the one of -a
    rc, out2, err2 = run(["--exclude", made["xgz"], made["fastq"]] + FLAG)
    assert rc == 0 and out2 == out and excluded_line(made) in err2 and b"  25 sequences, %d canonical 24-mers\n\n" % made["keys"] in err2
    # --exclude_percent 60: only the clean copies keep 60 % of their 24-mers
    rc, out60, err60 = run(["--exclude", made["x"], "--exclude_percent", "60", made["fastq"]] + FLAG, SMALL_BATCHES)
    assert rc == 0 and out60 == without(plain, names(made, 60.0)) and excluded_line(made, 60.0) in err60
    assert b"@read_0\n" in out60 and b"@read_0\n" not in out


def test_verbose_lines(made):
    rc, out, err = run(["--exclude", made["x"], "--min_length", "1", "--verbose", made["fastq"]] + FLAG, SMALL_BATCHES)
    assert rc == 0 and names(made)
    got = re.findall(rb"\n(\S+)\n +length = [^\n]*\n          excluded = (yes|no) \((\d+) of (\d+) 24-mers\)\n", err)
    want = [(n, b"yes" if e else b"no", b"%d" % h, b"%d" % (len(s) - K + 1)) for (n, s, _), e, h in zip(made["reads"], made[10.0], made["hits"])]
    assert got == want
    assert excluded_line(made) in err


def test_keep_percent_over_the_flags_with_the_excluded_failing(made):
    reads = made["reads"]
    assert names(made)
    p = _oracle.make_params(window_size=250)
    sc = [_oracle.score_read(None, q, p) for _, _, q in reads]
    passed = np.array([0 if e else s["passed"] for s, e in zip(sc, made[10.0])], dtype=np.uint8)
    total = sum(len(s) for _, s, _ in reads)
    r = _oracle.rank_and_cut(np.array([s["mean_q"] for s in sc]), np.array([s["window_q"] for s in sc]),
                             np.array([len(s) for _, s, _ in reads], dtype=np.int32), passed, keep_percent=70.0, total_bases=total)
    want = fastq_bytes([x for x, keep in zip(reads, r["passed"]) if keep])
    rc, out, err = run(["--exclude", made["x"], "--keep_percent", "70", made["fastq"]] + FLAG, SMALL_BATCHES)
    assert rc == 0 and out == want
    assert b"  target: %d bp\n" % int(0.7 * total) in err  # of the INPUT's bases
    assert 0 < len(records(out)) <= 40
    rc, out2, err2 = run(["--exclude", made["x"], "--keep_percent", "70", "--gpus", "2", made["fastq"]] + FLAG, dict(shim_env(), **SMALL_BATCHES))
    assert rc == 0 and out2 == want and excluded_line(made) in err2


def test_the_same_reads_by_every_road(made):
    rc, plain, _ = run(["--min_length", "1", made["fastq"]])
    want = without(plain, names(made))
    args = ["--exclude", made["x"], "--min_length", "1"] + FLAG
    rc, out, err = run(args + [made["gz"]], dict(SMALL_BATCHES, FLX_CLI_BLOCK_BYTES="20000", FLX_CLI_CHUNK_BYTES="30000"))  # streamed, many chunks
    assert rc == 0 and out == want and excluded_line(made) in err
    rc, out, err = run(args + [made["bam"]], SMALL_BATCHES)
    assert rc == 0 and out == want and excluded_line(made) in err
    rc, out, err = run(args + ["--gzip", made["fastq"]], SMALL_BATCHES)
    assert rc == 0 and gzip.decompress(out) == want
    rc, out, err = run(args + ["--bam", made["fastq"]], SMALL_BATCHES)
    assert rc == 0
    data, info = _bgzf.validate(out)
    recs, end = _bam.walk_model(data)
    assert info["eof"] and end == _bam.END and _bam.expected_fastq(recs)[0] == want
    rc, out, err = run(args + ["--gpus", "2", made["fastq"]], dict(shim_env(), **SMALL_BATCHES))
    assert rc == 0 and out == want and excluded_line(made) in err
    rc, out, err = run(args + ["--gpus", "2", "--verbose", made["fastq"]], dict(shim_env(), **SMALL_BATCHES))
    assert rc == 0 and out == want and err.count(b"          excluded = yes") == 20 and err.count(b"          excluded = no") == 40


def test_children_of_an_excluded_parent(made):
    excluded = names(made)
    # k-mer mode with --trim --split: the one plane serves the scoring and the screen; the chimera's children go with it
    kmer = ["-a", made["g"], "--trim", "--split", "100", "--min_length", "50"]
    rc, plain, err0 = run(kmer + [made["fastq"]])
    assert rc == 0 and re.search(rb"^@read_0_\d+-\d+$", plain, re.M), "the chimera has a child without the flag"
    rc, out, err = run(kmer + ["--exclude", made["x"], made["fastq"]] + FLAG, SMALL_BATCHES)
    assert rc == 0 and out == without(plain, excluded) and excluded_line(made) in err
    assert not re.search(rb"^@read_0(_\d+-\d+)?$", out, re.M) and len(out) > 0
    assert err.index(excluded_line(made)) < err.index(b"  after trimming and splitting: ")
    # Phred mode with --split_window_q: two planes a chunk
    qs = ["--split_window_q", "85"]
    rc, plain, _ = run(qs + [made["fastq"]])
    assert rc == 0 and re.search(rb"^@read_6_\d+-\d+$", plain, re.M), "an excluded read splits without the flag"
    rc, out, err = run(qs + ["--exclude", made["x"], made["fastq"]] + FLAG, dict(SMALL_BATCHES, FLX_CLI_CHUNK_BYTES="30000"))
    assert rc == 0 and out == without(plain, excluded) and excluded_line(made) in err
    assert not re.search(rb"^@read_6(_\d+-\d+)?$", out, re.M) and re.search(rb"^@read_1_\d+-\d+$", out, re.M)


def test_report(made, tmp_path):
    from filtlong_amd import api
    assert names(made)
    rep, rep0 = tmp_path / "r.json", tmp_path / "r0.json"
    rc, out, err = run(["--exclude", made["x"], "--min_length", "1", "--report", str(rep), made["fastq"]] + FLAG, SMALL_BATCHES)
    assert rc == 0
    rc, out0, err0 = run(["--min_length", "1", "--report", str(rep0), made["fastq"]])
    assert rc == 0
    got, got0 = json.loads(rep.read_bytes()), json.loads(rep0.read_bytes())
    assert list(got) == ["version", "q_edges", "input", "scored", "kept", "excluded"] and got["input"] == got0["input"]
    reads = made["reads"]
    p = _oracle.make_params(window_size=250)
    sc = [_oracle.score_read(None, q, p) for _, _, q in reads]
    ctx = api.Context(0)
    try:
        want = ctx.summary([len(s) for _, s, _ in reads], [s["mean_q"] for s in sc], [s["window_q"] for s in sc], mask=np.array(made[10.0], dtype=np.uint8))
    finally:
        ctx.close()
    assert got["excluded"] == want and got["excluded"]["n"] == 20
    assert got["kept"]["n"] == 40 and got0["kept"]["n"] == 60


def test_exclude_k_16_is_the_run_without_the_flag(made, tmp_path):
    """stdout, stderr and the report, byte for byte: the bitmap path runs"""
    rep, rep16 = tmp_path / "r.json", tmp_path / "r16.json"
    args = ["--exclude", made["x"], "--min_length", "1", "--verbose"]
    rc, out, err = run(args + ["--report", str(rep), made["fastq"]])
    rc16, out16, err16 = run(args + ["--report", str(rep16), "--exclude_k", "16", made["fastq"]])
    assert rc == rc16 == 0 and out16 == out and err16 == err and rep16.read_bytes() == rep.read_bytes()
    assert b"Hashing 16-mers to exclude\n" in err and b"canonical" not in err and b" 16-mers)\n" in err
    assert 0 < len(records(out)) < 60


def test_too_many_17_mers(made, tmp_path):
    ref = model.random_seq(np.random.default_rng(4), 2000)
    fa = tmp_path / "small.fa"
    fa.write_bytes(b">small\n" + ref + b"\n")
    n = len(model.build_set([ref], 17))
    assert n == 2000 - 16 and n * 400 >= 0.00001 * 4 ** 17 and n * 400 < 10 * 4 ** 17
    rc, out, err = run(["--exclude", str(fa), "--exclude_k", "17", "--exclude_percent", "0.00001", made["fastq"]])
    assert rc == 1 and out == b""
    assert err.endswith(b"Error: the reference for --exclude holds too many 17-mers (%d) for --exclude_percent 0.00001\n" % n)
    # at the default 10 % the same reference is fine (and excludes nothing here)
    rc, out, err = run(["--exclude", str(fa), "--exclude_k", "17", "--min_length", "1", made["fastq"]])
    assert rc == 0 and out == fastq_bytes(made["reads"]) and b"  excluded by reference: 0 reads (0 bp)\n" in err
    # a reference without a K-mer of ACGT
    fa.write_bytes(b">none\n" + ref[:23] + b"N" + ref[:23] + b"\n")
    rc, out, err = run(["--exclude", str(fa), "--exclude_k", "24", made["fastq"]])
    assert rc == 1 and out == b"" and err.endswith(b"Error: the reference for --exclude holds no 24-mer of ACGT\n")
