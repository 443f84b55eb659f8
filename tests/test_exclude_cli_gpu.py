"""--exclude through the whole command line, against tests/_screen_model.py: stdout is the run without the flag minus exactly the reads
the model excludes (and the children of those), the "excluded by reference" line, the --verbose lines and --report's fourth summary
are the model's, with a cut the kept reads are the oracle's rank_and_cut over the flags with the excluded reads failing, and a streamed
gzip input, a BAM input, --gzip, --bam, --gpus 2, k-mer mode with --trim --split and --split_window_q all give the same reads."""
import gzip
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import _bam
import _bgzf
import _oracle
import _qsplit_model as qmodel
import _screen_model as model

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "filtlong_amd", "bin", "filtlong")
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_bam  # noqa: E402  (the BAM writer of tools/gen_bam.py)


def run(args, extra=None):
    env = dict(os.environ, LANG="C", LC_ALL="C")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    env.update(extra or {})
    p = subprocess.run([BIN] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
    return p.returncode, p.stdout, p.stderr


def shim_env():
    shim_dir = os.path.join(ROOT, "tests", "shim")
    subprocess.check_call(["make", "-s", "-C", shim_dir])
    return {"FLX_RCCL_LIB": os.path.join(shim_dir, "libloopback_rccl.so"), "FLX_DEVICE": "0"}


def fastq_bytes(reads):
    return b"".join(b"@" + n + b"\n" + s + b"\n+\n" + q + b"\n" for n, s, q in reads)


def records(text):
    """FASTQ text -> [(name, the record's bytes)]"""
    lines = text.split(b"\n")
    assert lines[-1] == b"" and (len(lines) - 1) % 4 == 0
    return [(lines[k][1:], b"\n".join(lines[k:k + 4]) + b"\n") for k in range(0, len(lines) - 1, 4)]


def without(text, excluded_names):
    """the records of `text` whose read — or, for a child name_start-end, whose parent — is not excluded"""
    keep = []
    for name, rec in records(text):
        parent = re.sub(rb"_\d+-\d+$", b"", name)
        if name not in excluded_names and parent not in excluded_names:
            keep.append(rec)
    return b"".join(keep)


@pytest.fixture(scope="module")
def made(tmp_path_factory):
    """60 reads: 20 from a 5 kbp contaminant (both strands, 5 % substitutions; read 0 is a chimera, half contaminant), 40 from a 60 kbp
    genome the contaminant has nothing to do with; some with a junk stretch in their qualities"""
    d = tmp_path_factory.mktemp("exclude_cli")
    rng = np.random.default_rng(909)
    xref, gref = model.random_seq(rng, 5000), model.random_seq(rng, 60000)
    reads = []
    for i in range(60):
        n = int(rng.integers(600, 4000))
        if i == 0:
            seq = model.draw(rng, gref, 1500, 0.02) + model.draw(rng, xref, 1500, 0.05)
        elif i % 3 == 0:
            seq = model.draw(rng, xref, n, 0.05)
        else:
            seq = model.draw(rng, gref, n, 0.02)
        st = [(len(seq) // 2, len(seq) // 2 + 350)] if i % 4 == 1 or i == 6 else []
        reads.append((b"read_%d" % i, seq, qmodel.junk_read(rng, len(seq), st, good=(25, 40), junk=(0, 3))))
    x_fa = b">lambda control\n" + xref[:2500] + b"\n" + xref[2500:3000] + b"NNNNNNNNNNNNNNNNNNNNNNNNN\n>second\n" + xref[3000:] + b"\n"
    (d / "x.fa").write_bytes(x_fa)
    (d / "x.fa.gz").write_bytes(gzip.compress(x_fa))
    (d / "g.fa").write_bytes(b">g\n" + gref + b"\n")
    (d / "made.fastq").write_bytes(fastq_bytes(reads))
    (d / "made.fastq.gz").write_bytes(gzip.compress(fastq_bytes(reads)))
    (d / "made.bam").write_bytes(gen_bam.bgzf(gen_bam.fastq_to_bam(fastq_bytes(reads))))
    x = model.build_set([xref[:3000], xref[3000:]])
    hits = [model.hits(x, s) for _, s, _ in reads]
    out = {"dir": d, "reads": reads, "x": str(d / "x.fa"), "xgz": str(d / "x.fa.gz"), "g": str(d / "g.fa"), "fastq": str(d / "made.fastq"),
           "gz": str(d / "made.fastq.gz"), "bam": str(d / "made.bam"), "hits": hits}
    for pct in (10.0, 60.0):
        out[pct] = [model.excluded(h, len(s), pct) for h, (_, s, _) in zip(hits, reads)]
    assert sum(out[10.0]) == 20 and out[10.0][0] and not out[60.0][0]
    return out


def names(made, pct=10.0):
    return {n for (n, _, _), e in zip(made["reads"], made[pct]) if e}


def excluded_line(made, pct=10.0):
    return b"  excluded by reference: %d reads (%d bp)\n" % (sum(made[pct]), sum(len(s) for (_, s, _), e in zip(made["reads"], made[pct]) if e))


def test_stdout_is_the_run_without_the_flag_minus_the_excluded(made):
    rc, plain, err0 = run(["--min_length", "1", made["fastq"]])
    assert rc == 0 and plain == fastq_bytes(made["reads"]) and b"excluded" not in err0
    rc, out, err = run(["--exclude", made["x"], "--min_length", "1", made["fastq"]])
    assert rc == 0 and b"Error" not in err, err[-2000:]
    assert out == without(plain, names(made)) and len(records(out)) == 40
    assert excluded_line(made) in err and err.index(excluded_line(made)) > err.index(b"60 reads")
    # the flag alone is a threshold; a gzip FASTA is read like the one of -a
    rc, out2, err2 = run(["--exclude", made["xgz"], made["fastq"]])
    assert rc == 0 and out2 == out and excluded_line(made) in err2
    # --exclude_percent 60: reads with 5 % substitutions keep 44 % of their 16-mers, the chimera 22 %: they stay
    rc, out60, err60 = run(["--exclude", made["x"], "--exclude_percent", "60", made["fastq"]])
    assert rc == 0 and out60 == without(plain, names(made, 60.0)) and excluded_line(made, 60.0) in err60
    assert b"@read_0\n" in out60 and b"@read_0\n" not in out


def test_verbose_lines(made):
    rc, out, err = run(["--exclude", made["x"], "--min_length", "1", "--verbose", made["fastq"]])
    assert rc == 0
    got = re.findall(rb"\n(\S+)\n +length = [^\n]*\n          excluded = (yes|no) \((\d+) of (\d+) 16-mers\)\n", err)
    want = [(n, b"yes" if e else b"no", b"%d" % h, b"%d" % (len(s) - 15)) for (n, s, _), e, h in zip(made["reads"], made[10.0], made["hits"])]
    assert got == want
    assert excluded_line(made) in err
    rc, _, err0 = run(["--min_length", "1", "--verbose", made["fastq"]])
    assert rc == 0 and b"excluded" not in err0


def test_keep_percent_over_the_flags_with_the_excluded_failing(made):
    reads = made["reads"]
    p = _oracle.make_params(window_size=250)
    sc = [_oracle.score_read(None, q, p) for _, _, q in reads]
    passed = np.array([0 if e else s["passed"] for s, e in zip(sc, made[10.0])], dtype=np.uint8)
    total = sum(len(s) for _, s, _ in reads)
    r = _oracle.rank_and_cut(np.array([s["mean_q"] for s in sc]), np.array([s["window_q"] for s in sc]),
                             np.array([len(s) for _, s, _ in reads], dtype=np.int32), passed, keep_percent=70.0, total_bases=total)
    want = fastq_bytes([x for x, keep in zip(reads, r["passed"]) if keep])
    rc, out, err = run(["--exclude", made["x"], "--keep_percent", "70", made["fastq"]])
    assert rc == 0 and out == want
    assert b"  target: %d bp\n" % int(0.7 * total) in err  # of the INPUT's bases
    assert 0 < len(records(out)) <= 40
    rc, out2, err2 = run(["--exclude", made["x"], "--keep_percent", "70", "--gpus", "2", made["fastq"]], shim_env())
    assert rc == 0 and out2 == want and excluded_line(made) in err2


def test_the_same_reads_by_every_road(made):
    rc, plain, _ = run(["--min_length", "1", made["fastq"]])
    want = without(plain, names(made))
    args = ["--exclude", made["x"], "--min_length", "1"]
    rc, out, err = run(args + [made["gz"]], {"FLX_CLI_BLOCK_BYTES": "20000", "FLX_CLI_CHUNK_BYTES": "30000"})  # streamed, many chunks
    assert rc == 0 and out == want and excluded_line(made) in err
    rc, out, err = run(args + [made["bam"]])
    assert rc == 0 and out == want and excluded_line(made) in err
    rc, out, err = run(args + ["--gzip", made["fastq"]])
    assert rc == 0 and gzip.decompress(out) == want
    rc, out, err = run(args + ["--bam", made["fastq"]])
    assert rc == 0
    data, info = _bgzf.validate(out)
    recs, end = _bam.walk_model(data)
    assert info["eof"] and end == _bam.END and _bam.expected_fastq(recs)[0] == want
    rc, out, err = run(args + ["--gpus", "2", made["fastq"]], shim_env())
    assert rc == 0 and out == want and excluded_line(made) in err
    rc, out, err = run(args + ["--gpus", "2", "--verbose", made["fastq"]], shim_env())
    assert rc == 0 and out == want and err.count(b"          excluded = yes") == 20 and err.count(b"          excluded = no") == 40


def test_children_of_an_excluded_parent(made):
    # k-mer mode with --trim --split: the one plane serves the scoring and the screen; the chimera's children go with it
    kmer = ["-a", made["g"], "--trim", "--split", "100", "--min_length", "50"]
    rc, plain, err0 = run(kmer + [made["fastq"]])
    assert rc == 0 and re.search(rb"^@read_0_\d+-\d+$", plain, re.M), "the chimera has a child without the flag"
    rc, out, err = run(kmer + ["--exclude", made["x"], made["fastq"]])
    assert rc == 0 and out == without(plain, names(made)) and excluded_line(made) in err
    assert not re.search(rb"^@read_0(_\d+-\d+)?$", out, re.M) and len(out) > 0
    assert err.index(excluded_line(made)) < err.index(b"  after trimming and splitting: ")
    # Phred mode with --split_window_q: two planes a chunk
    qs = ["--split_window_q", "85"]
    rc, plain, _ = run(qs + [made["fastq"]])
    assert rc == 0 and re.search(rb"^@read_6_\d+-\d+$", plain, re.M), "an excluded read splits without the flag"
    rc, out, err = run(qs + ["--exclude", made["x"], made["fastq"]], {"FLX_CLI_CHUNK_BYTES": "30000"})
    assert rc == 0 and out == without(plain, names(made)) and excluded_line(made) in err
    assert not re.search(rb"^@read_6(_\d+-\d+)?$", out, re.M) and re.search(rb"^@read_1_\d+-\d+$", out, re.M)


def test_report(made, tmp_path):
    from filtlong_amd import api
    rep, rep0 = tmp_path / "r.json", tmp_path / "r0.json"
    rc, out, err = run(["--exclude", made["x"], "--min_length", "1", "--report", str(rep), made["fastq"]])
    assert rc == 0
    rc, out0, err0 = run(["--min_length", "1", "--report", str(rep0), made["fastq"]])
    assert rc == 0
    got, got0 = json.loads(rep.read_bytes()), json.loads(rep0.read_bytes())
    assert list(got0) == ["version", "q_edges", "input", "scored", "kept"] and got0["version"] == 1
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
    # ... and two ranks give the bytes of one
    rep2 = tmp_path / "r2.json"
    rc, out2, _ = run(["--exclude", made["x"], "--min_length", "1", "--report", str(rep2), "--gpus", "2", made["fastq"]], shim_env())
    assert rc == 0 and out2 == out and rep2.read_bytes() == rep.read_bytes()


def test_too_many_16_mers(made, tmp_path):
    big = model.random_seq(np.random.default_rng(4), 3000000)
    fa = tmp_path / "big.fa"
    fa.write_bytes(b">big\n" + big + b"\n")
    n = len(model.build_set([big]))
    assert n * 200 >= 0.1 * 2 ** 32 and n * 200 < 10 * 2 ** 32
    rc, out, err = run(["--exclude", str(fa), "--exclude_percent", "0.1", made["fastq"]])
    assert rc == 1 and out == b""
    assert err.endswith(b"Error: the reference for --exclude holds too many 16-mers (%d) for --exclude_percent 0.1\n" % n)
    # at the default 10 % the same reference is fine (and excludes nothing here)
    rc, out, err = run(["--exclude", str(fa), "--min_length", "1", made["fastq"]])
    assert rc == 0 and out == fastq_bytes(made["reads"]) and b"  excluded by reference: 0 reads (0 bp)\n" in err
