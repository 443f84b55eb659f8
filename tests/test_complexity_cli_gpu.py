"""--max_low_complexity through the whole command line, against tests/_complexity_model.py: stdout is the run without the flag minus
exactly the reads the model flags (and the children of those), the "low complexity" line, the --verbose lines and --report's
"low_complexity" summary are the model's, with a cut the kept reads are the oracle's rank_and_cut over the flags with the flagged
reads failing, and a streamed gzip input, a BAM input, a FASTA input, --gzip, --bam, --gpus 2, k-mer mode with --trim --split,
--split_window_q, --trim_adapters --split_adapters and --exclude all give the same reads.  Without the flag stdout, stderr and the
report are what the oracle gives: the reads, the reference binary's stderr, and the summaries of tests/_summary.py."""
import gzip
import json
import os
import re
import sys

import numpy as np
import pytest

import _adapters_cases as acases
import _bam
import _bgzf
import _complexity_model as model
import _oracle
import _qsplit_model as qmodel
import _screen_model as smodel
import _summary
from test_exclude_cli_gpu import fastq_bytes, records, run, shim_env, without

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_bam  # noqa: E402  (the BAM writer of tools/gen_bam.py)

P = 50.0


@pytest.fixture(scope="module")
def made(tmp_path_factory):
    """60 reads with good qualities: 20 repeat junk (period 1..6, 3 % substitutions but in the homopolymers), two chimeras that are
    half junk (read_1 above 50 % of its windows, read_2 below), four from a 5 kbp contaminant, some with an adapter at the head or in
    the middle, the rest from a 60 kbp genome; some with a junk stretch in their qualities"""
    d = tmp_path_factory.mktemp("complexity_cli")
    rng = np.random.default_rng(606)
    xref, gref = smodel.random_seq(rng, 5000), smodel.random_seq(rng, 60000)
    reads = []
    for i in range(60):
        n = int(rng.integers(600, 4000))
        if i == 1:
            seq = smodel.draw(rng, gref, 800, 0.0, 0) + model.repeat(rng, 2, 1500)
        elif i == 2:
            seq = smodel.draw(rng, gref, 1500, 0.0, 0) + model.repeat(rng, 3, 900)
        elif i % 3 == 0:
            seq = model.repeat(rng, 1 + i // 3 % 6, n, rate=0.03 if i // 3 % 6 else 0.0)  # (the homopolymers are exact: bad at score 300 too)
        elif i % 10 == 4:
            seq = smodel.draw(rng, xref, min(n, 3000), 0.03)
        elif i % 10 == 7:
            seq = acases.LIGATION + smodel.draw(rng, gref, n, 0.02)
        elif i == 5:
            seq = smodel.draw(rng, gref, 1200, 0.02) + acases.LIGATION + smodel.draw(rng, gref, 1000, 0.02)
        else:
            seq = smodel.draw(rng, gref, n, 0.02)
        if i == 9:
            seq = acases.LIGATION + seq  # a flagged read with an adapter: its trimmed child goes with it
        st = [(len(seq) // 2, len(seq) // 2 + 350)] if i % 4 == 1 or i == 6 else []
        reads.append((b"read_%d" % i, seq, qmodel.junk_read(rng, len(seq), st, good=(25, 40), junk=(0, 3))))
    (d / "x.fa").write_bytes(b">x\n" + xref + b"\n")
    (d / "g.fa").write_bytes(b">g\n" + gref + b"\n")
    (d / "adapters.fa").write_bytes(b">ligation\n" + acases.LIGATION + b"\n")
    (d / "made.fastq").write_bytes(fastq_bytes(reads))
    (d / "made.fastq.gz").write_bytes(gzip.compress(fastq_bytes(reads)))
    (d / "made.bam").write_bytes(gen_bam.bgzf(gen_bam.fastq_to_bam(fastq_bytes(reads))))
    (d / "made.fasta").write_bytes(b"".join(b">" + n + b"\n" + s + b"\n" for n, s, _ in reads))
    seqs = [s for _, s, _ in reads]
    out = {"dir": d, "reads": reads, "x": str(d / "x.fa"), "g": str(d / "g.fa"), "ad": str(d / "adapters.fa"), "fastq": str(d / "made.fastq"),
           "gz": str(d / "made.fastq.gz"), "bam": str(d / "made.bam"), "fasta": str(d / "made.fasta")}
    for T in (20, 300):
        out["bad", T] = model.bad_many(seqs, T)
    for pct in (P, 90.0):
        out[pct] = [bool(f) for f in model.flagged_many(out["bad", 20], [len(s) for s in seqs], pct)]
    out["T300"] = [bool(f) for f in model.flagged_many(out["bad", 300], [len(s) for s in seqs], P)]
    assert sum(out[P]) == 21 and out[P][1] and not out[P][2] and out["bad", 20][2] > 500 and not out[90.0][1]
    assert 0 < sum(out["T300"]) < 10  # only the homopolymer reads
    x = smodel.build_set([xref])
    out["excl"] = [smodel.excluded(smodel.hits(x, s), len(s), 10.0) for s in seqs]
    assert sum(out["excl"]) == 4 and not any(a and b for a, b in zip(out["excl"], out[P]))
    return out


def names(made, key=P):
    return {n for (n, _, _), e in zip(made["reads"], made[key]) if e}


def low_line(made, key=P):
    return b"  low complexity: %d reads (%d bp)\n" % (sum(made[key]), sum(len(s) for (_, s, _), e in zip(made["reads"], made[key]) if e))


def test_stdout_is_the_run_without_the_flag_minus_the_flagged(made):
    rc, plain, err0 = run(["--min_length", "1", made["fastq"]])
    assert rc == 0 and plain == fastq_bytes(made["reads"]) and b"complexity" not in err0
    rc, out, err = run(["--max_low_complexity", "50", "--min_length", "1", made["fastq"]])
    assert rc == 0 and b"Error" not in err, err[-2000:]
    assert out == without(plain, names(made)) and len(records(out)) == 39
    assert low_line(made) in err and err.index(low_line(made)) > err.index(b"60 reads")
    assert b"@read_2\n" in out and b"@read_1\n" not in out  # the two chimeras
    # the flag alone is a threshold
    rc, out2, err2 = run(["--max_low_complexity", "50", made["fastq"]])
    assert rc == 0 and out2 == out and low_line(made) in err2
    # 90 %: the chimera above 50 % stays; score 300: only homopolymer windows are bad
    rc, out90, err90 = run(["--max_low_complexity", "90", made["fastq"]])
    assert rc == 0 and out90 == without(plain, names(made, 90.0)) and low_line(made, 90.0) in err90 and b"@read_1\n" in out90
    rc, out300, err300 = run(["--max_low_complexity", "50", "--low_complexity_score", "300", made["fastq"]])
    assert rc == 0 and out300 == without(plain, names(made, "T300")) and low_line(made, "T300") in err300


def test_verbose_lines(made):
    rc, out, err = run(["--max_low_complexity", "50", "--min_length", "1", "--verbose", made["fastq"]])
    assert rc == 0
    got = re.findall(rb"\n(\S+)\n +length = [^\n]*\n          low complexity = (yes|no) \((\d+) of (\d+) windows\)\n", err)
    want = [(n, b"yes" if e else b"no", b"%d" % b, b"%d" % (len(s) - 63)) for (n, s, _), e, b in zip(made["reads"], made[P], made["bad", 20])]
    assert got == want
    assert low_line(made) in err
    rc, _, err0 = run(["--min_length", "1", "--verbose", made["fastq"]])
    assert rc == 0 and b"complexity" not in err0
    # behind the excluded line of the same read
    rc, _, err = run(["--max_low_complexity", "50", "--exclude", made["x"], "--min_length", "1", "--verbose", made["fastq"]])
    assert rc == 0
    both = re.findall(rb"          excluded = (yes|no) \(\d+ of \d+ 16-mers\)\n          low complexity = (yes|no) \((\d+) of \d+ windows\)\n", err)
    assert both == [(b"yes" if x else b"no", b"yes" if e else b"no", b"%d" % b) for x, e, b in zip(made["excl"], made[P], made["bad", 20])]


def test_keep_percent_over_the_flags_with_the_flagged_failing(made):
    reads = made["reads"]
    p = _oracle.make_params(window_size=250)
    sc = [_oracle.score_read(None, q, p) for _, _, q in reads]
    passed = np.array([0 if e else s["passed"] for s, e in zip(sc, made[P])], dtype=np.uint8)
    total = sum(len(s) for _, s, _ in reads)
    r = _oracle.rank_and_cut(np.array([s["mean_q"] for s in sc]), np.array([s["window_q"] for s in sc]),
                             np.array([len(s) for _, s, _ in reads], dtype=np.int32), passed, keep_percent=60.0, total_bases=total)
    want = fastq_bytes([x for x, keep in zip(reads, r["passed"]) if keep])
    rc, out, err = run(["--max_low_complexity", "50", "--keep_percent", "60", made["fastq"]])
    assert rc == 0 and out == want
    assert b"  target: %d bp\n" % int(0.6 * total) in err  # of the INPUT's bases
    assert 0 < len(records(out)) <= 39
    rc, out2, err2 = run(["--max_low_complexity", "50", "--keep_percent", "60", "--gpus", "2", made["fastq"]], shim_env())
    assert rc == 0 and out2 == want and low_line(made) in err2


def test_the_same_reads_by_every_road(made):
    rc, plain, _ = run(["--min_length", "1", made["fastq"]])
    want = without(plain, names(made))
    args = ["--max_low_complexity", "50", "--min_length", "1"]
    rc, out, err = run(args + [made["gz"]], {"FLX_CLI_BLOCK_BYTES": "20000", "FLX_CLI_CHUNK_BYTES": "30000"})  # streamed, many chunks
    assert rc == 0 and out == want and low_line(made) in err
    rc, out, err = run(args + [made["bam"]])
    assert rc == 0 and out == want and low_line(made) in err
    fa = ["-a", made["g"], "--min_length", "1"]  # (FASTA input has no qualities: it needs an external reference)
    rc, plain_fa, _ = run(fa + [made["fasta"]])
    rc2, out, err = run(fa + ["--max_low_complexity", "50", made["fasta"]])
    assert rc == 0 and rc2 == 0 and low_line(made) in err and out.count(b">") == 39
    assert plain_fa == b"".join(b">" + n + b"\n" + s + b"\n" for n, s, _ in made["reads"])
    assert out == b"".join(b">" + n + b"\n" + s + b"\n" for (n, s, _), e in zip(made["reads"], made[P]) if not e)
    rc, out, err = run(args + ["--gzip", made["fastq"]])
    assert rc == 0 and gzip.decompress(out) == want
    rc, out, err = run(args + ["--bam", made["fastq"]])
    assert rc == 0
    data, info = _bgzf.validate(out)
    recs, end = _bam.walk_model(data)
    assert info["eof"] and end == _bam.END and _bam.expected_fastq(recs)[0] == want
    rc, out, err = run(args + ["--gpus", "2", made["fastq"]], shim_env())
    assert rc == 0 and out == want and low_line(made) in err
    rc, out, err = run(args + ["--gpus", "2", "--verbose", made["fastq"]], shim_env())
    assert rc == 0 and out == want and err.count(b"          low complexity = yes") == 21 and err.count(b"          low complexity = no") == 39


def test_children_of_a_flagged_parent(made):
    flag = ["--max_low_complexity", "50"]
    # k-mer mode with --trim --split: the one plane serves the scoring and the filter; the chimera's child goes with it
    kmer = ["-a", made["g"], "--trim", "--split", "100", "--min_length", "50"]
    rc, plain, err0 = run(kmer + [made["fastq"]])
    assert rc == 0 and re.search(rb"^@read_1_\d+-\d+$", plain, re.M), "the chimera has a child without the flag"
    rc, out, err = run(kmer + flag + [made["fastq"]])
    assert rc == 0 and out == without(plain, names(made)) and low_line(made) in err
    assert not re.search(rb"^@read_1(_\d+-\d+)?$", out, re.M) and re.search(rb"^@read_2(_\d+-\d+)?$", out, re.M)
    assert err.index(low_line(made)) < err.index(b"  after trimming and splitting: ")
    # Phred mode with --split_window_q: two planes a chunk
    qs = ["--split_window_q", "85"]
    rc, plain, _ = run(qs + [made["fastq"]])
    assert rc == 0 and re.search(rb"^@read_6_\d+-\d+$", plain, re.M), "a flagged read splits without the flag"
    rc, out, err = run(qs + flag + [made["fastq"]], {"FLX_CLI_CHUNK_BYTES": "30000"})
    assert rc == 0 and out == without(plain, names(made)) and low_line(made) in err
    assert not re.search(rb"^@read_6(_\d+-\d+)?$", out, re.M) and re.search(rb"^@read_5_\d+-\d+$", out, re.M)
    # --trim_adapters --split_adapters: the filter looks at the whole parent; a flagged parent's trimmed child fails
    ta = ["--trim_adapters", made["ad"], "--split_adapters", "--min_length", "1"]
    rc, plain, _ = run(ta + [made["fastq"]])
    assert rc == 0 and re.search(rb"^@read_9_\d+-\d+$", plain, re.M) and len(re.findall(rb"^@read_5_\d+-\d+$", plain, re.M)) == 2
    rc, out, err = run(ta + flag + [made["fastq"]])
    assert rc == 0 and out == without(plain, names(made)) and low_line(made) in err
    assert not re.search(rb"^@read_9(_\d+-\d+)?$", out, re.M) and err.index(low_line(made)) < err.index(b"  split at adapters: ")


def test_together_with_exclude(made):
    rc, plain, _ = run(["--min_length", "1", made["fastq"]])
    gone = names(made) | names(made, "excl")
    assert len(gone) == 25
    excl_line = b"  excluded by reference: 4 reads (%d bp)\n" % sum(len(s) for (_, s, _), e in zip(made["reads"], made["excl"]) if e)
    for extra in ([], ["--exclude_k", "21"]):
        rc, out, err = run(["--max_low_complexity", "50", "--exclude", made["x"], "--min_length", "1"] + extra + [made["fastq"]])
        assert rc == 0 and out == without(plain, gone)
        assert excl_line + low_line(made) in err  # directly behind it


def summary_text(s):
    return json.dumps({k: s[k] for k in _summary.FIELDS})


def report_text(summaries):
    edges = ", ".join("%.17g" % e for e in _summary.api.summary_q_edges())
    return ('{"version": 1, "q_edges": [' + edges + "]" + "".join(',\n "%s": %s' % (k, summary_text(v)) for k, v in summaries) + "}\n").encode()


def oracle_summaries(made, masks):
    reads = made["reads"]
    p = _oracle.make_params(window_size=250)
    sc = [_oracle.score_read(None, q, p) for _, _, q in reads]
    ln, mq, wq = [len(s) for _, s, _ in reads], [s["mean_q"] for s in sc], [s["window_q"] for s in sc]
    return [(k, _summary.reference(ln, mq, wq, None if m is None else np.array(m, dtype=np.uint8))) for k, m in masks]


def test_report(made, tmp_path):
    rep = tmp_path / "r.json"
    rc, out, err = run(["--max_low_complexity", "50", "--min_length", "1", "--report", str(rep), made["fastq"]])
    assert rc == 0
    got = json.loads(rep.read_bytes())
    assert list(got) == ["version", "q_edges", "input", "scored", "kept", "low_complexity"]
    keep = [not e for e in made[P]]
    assert rep.read_bytes() == report_text(oracle_summaries(made, [("input", None), ("scored", None), ("kept", keep), ("low_complexity", made[P])]))
    assert got["low_complexity"]["n"] == 21 and got["kept"]["n"] == 39
    # behind "excluded" when both flags are given
    rc, out, err = run(["--max_low_complexity", "50", "--exclude", made["x"], "--min_length", "1", "--report", str(rep), made["fastq"]])
    assert rc == 0
    got = json.loads(rep.read_bytes())
    assert list(got) == ["version", "q_edges", "input", "scored", "kept", "excluded", "low_complexity"]
    keep = [not (e or x) for e, x in zip(made[P], made["excl"])]
    assert rep.read_bytes() == report_text(oracle_summaries(made, [("input", None), ("scored", None), ("kept", keep), ("excluded", made["excl"]),
                                                                   ("low_complexity", made[P])]))
    # ... and two ranks give the bytes of one
    rep2 = tmp_path / "r2.json"
    rc, out2, _ = run(["--max_low_complexity", "50", "--exclude", made["x"], "--min_length", "1", "--report", str(rep2), "--gpus", "2", made["fastq"]],
                      shim_env())
    assert rc == 0 and out2 == out and rep2.read_bytes() == rep.read_bytes()


def test_without_the_flag_every_byte_is_what_it_was(made, tmp_path):
    """stdout is the input (every read passes --min_length 1), stderr the reference binary's for the same command, the report the
    three summaries of tests/_summary.py over the oracle's scores: nothing of the filter shows"""
    if not _oracle.have_ref():
        pytest.fail("oracle/_ref is not built: build() makes the reference binary")
    rep = tmp_path / "r0.json"
    rc, out, err = run(["--min_length", "1", "--report", str(rep), made["fastq"]])
    rrc, rout, rerr = _oracle.run_ref_filtlong(["--min_length", "1", made["fastq"]])
    assert rc == 0 and rrc == 0
    assert out == fastq_bytes(made["reads"]) and out == rout
    assert err == rerr.encode()
    assert rep.read_bytes() == report_text(oracle_summaries(made, [("input", None), ("scored", None), ("kept", None)]))
    rc, out, err = run(["--min_length", "1", "--verbose", made["fastq"]])
    rrc, rout, rerr = _oracle.run_ref_filtlong(["--min_length", "1", "--verbose", made["fastq"]])
    assert rc == 0 and rrc == 0 and out == rout and err == rerr.encode()
