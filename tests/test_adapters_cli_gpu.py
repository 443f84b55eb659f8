"""--trim_adapters through the whole command line, against tests/_adapters_model.py: stdout holds the model's trimmed records, named
name_start-end like the children of --trim, and the untouched reads whole; a read of which nothing is left is gone; the "after adapter
trimming" line, the --verbose lines and --report's scored summary are the model's; with --keep_percent the kept reads are those of the
oracle's rank_and_cut over the model's children; a streamed gzip input, a BAM input, --gzip, --bam and --gpus 2 give the same reads;
without the flag every byte is what it was."""
import gzip
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import _adapters_cases as cases
import _adapters_model as model
import _bam
import _bgzf
import _oracle
from filtlong_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "filtlong_amd", "bin", "filtlong")
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_bam  # noqa: E402  (the BAM writer of tools/gen_bam.py)

NAMES = [b"ligation_top", b"second"]
SEQS = [cases.LIGATION, b"GGTTGTTTCTGTTGGTGCTGATATTGC"]
WINDOW, ERRORS = 150, 20


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


class Expected:
    def __init__(self, reads, window=WINDOW, errors=ERRORS):
        self.reads = reads
        self.keys = model.keys_of([s for _, s, _ in reads], window, model.patterns(SEQS), errors)

    def entries(self):
        """reads2: (name, seq, qual, may pass) — the child in place of its parent; a read of which nothing is left stays and fails"""
        out = []
        for (n, s, q), (kh, kt) in zip(self.reads, self.keys):
            ch, first, last = model.child_of(len(s), kh, kt)
            if not ch:
                out.append((n, s, q, first != -1))
            for st, en in ch:
                out.append((n + b"_%d-%d" % (st + 1, en), s[st:en], q[st:en], True))
        return out

    def stdout(self, min_length=1, upper=False):
        """upper: what comes back through BAM, whose 4-bit bases know no lower case"""
        return fastq_bytes([(n, s.upper() if upper else s, q) for n, s, q, ok in self.entries() if ok and len(s) >= min_length])

    def after_line(self):
        e = self.entries()
        return b"  after adapter trimming: %d reads (%d bp)\n" % (len(e), sum(len(s) for _, s, _, _ in e))

    def verbose_lines(self):
        def who(k):
            return NAMES[(int(k) & 255) >> 1] if k else b"none"
        return [b"          adapters = start %d (%s), end %d (%s)\n" % (int(kh) >> 8, who(kh), int(kt) >> 8, who(kt)) for kh, kt in self.keys]


@pytest.fixture(scope="module")
def made(tmp_path_factory):
    """60 short reads: adapters at the head, the tail, both, neither; with substitutions and indels; one that is all adapter"""
    d = tmp_path_factory.mktemp("adapters_cli")
    rng = np.random.default_rng(515)
    reads = []
    for i in range(60):
        n = int(rng.integers(200, 1500))
        body = cases.random_seq(rng, n)
        a = SEQS[i % 2]
        head = cases.random_seq(rng, int(rng.integers(0, 20))) + (cases.substitute(rng, a, 2) if i % 5 else cases.indel(rng, a, 2)) if i % 4 in (0, 1) else b""
        tail = model.revcomp(SEQS[(i // 2) % 2]) + cases.random_seq(rng, int(rng.integers(0, 12))) if i % 4 in (1, 2) else b""
        seq = head + body + tail
        if i == 13:
            seq = SEQS[0] + model.revcomp(SEQS[1])
        if i == 14:
            seq = seq.lower()
        reads.append((b"read_%d" % i, seq, synth.qual_read(4000 + i, len(seq)).tobytes()))
    fa = b"".join(b">" + n + b" a comment\n" + s + b"\n" for n, s in zip(NAMES, SEQS))
    (d / "adapters.fa").write_bytes(fa)
    (d / "adapters.fa.gz").write_bytes(gzip.compress(fa))
    (d / "made.fastq").write_bytes(fastq_bytes(reads))
    (d / "made.fastq.gz").write_bytes(gzip.compress(fastq_bytes(reads)))
    (d / "made.bam").write_bytes(gen_bam.bgzf(gen_bam.fastq_to_bam(fastq_bytes(reads))))
    want = Expected(reads)
    cut = want.keys >> 8
    assert (cut[:, 0] > 0).sum() >= 25 and (cut[:, 1] > 0).sum() >= 25 and ((cut[:, 0] == 0) & (cut[:, 1] == 0)).sum() >= 10
    assert any(not ok for _, _, _, ok in want.entries())
    return {"dir": d, "reads": reads, "fa": str(d / "adapters.fa"), "fagz": str(d / "adapters.fa.gz"), "fastq": str(d / "made.fastq"),
            "gz": str(d / "made.fastq.gz"), "bam": str(d / "made.bam"), "want": want}


def test_stdout_is_the_trimmed_reads(made):
    want = made["want"]
    rc, out, err = run(["--trim_adapters", made["fa"], made["fastq"]])
    assert rc == 0 and b"Error" not in err, err[-2000:]
    assert out == want.stdout()
    assert want.after_line() in err and b"Reading adapters\n  " + made["fa"].encode() + b"\n  2 sequences\n\n" in err
    assert err.index(b"Reading adapters") < err.index(b"Scoring long reads") < err.index(want.after_line())
    # a gzip FASTA is read like the one of -a; with a hard cut-off the children are judged as reads of their own
    rc, out2, _ = run(["--trim_adapters", made["fagz"], "--min_length", "600", made["fastq"]])
    assert rc == 0 and out2 == want.stdout(min_length=600) and out2 != out
    # --adapter_window / --adapter_errors reach the kernel
    narrow = Expected(made["reads"], window=30, errors=0)
    rc, out3, err3 = run(["--trim_adapters", made["fa"], "--adapter_window", "30", "--adapter_errors", "0", made["fastq"]])
    assert rc == 0 and out3 == narrow.stdout() and out3 != out and narrow.after_line() in err3


def test_without_the_flag_nothing_changes(made):
    rc, out, err = run(["--min_length", "1", made["fastq"]])
    assert rc == 0 and out == fastq_bytes(made["reads"])
    assert b"adapter" not in err.lower() and b"after" not in err
    rc, _, verr = run(["--min_length", "1", "--verbose", made["fastq"]])
    assert rc == 0 and b"adapters" not in verr


def test_verbose_lines(made):
    want = made["want"]
    rc, out, err = run(["--trim_adapters", made["fa"], "--verbose", made["fastq"]])
    assert rc == 0 and out == want.stdout()
    got = re.findall(rb"^          adapters = [^\n]*\n", err, re.M)
    assert got == want.verbose_lines()
    # the block of a trimmed read: bad ranges, child ranges, the adapters' line, then the child's own block
    (n, s, q), (kh, kt) = made["reads"][1], want.keys[1]
    st, en = int(kh) >> 8, len(s) - (int(kt) >> 8)
    assert st > 0 and en < len(s)
    block = b"        bad ranges = 0-%d, %d-%d\n      child ranges = %d-%d\n" % (st, en, len(s), st, en) + want.verbose_lines()[1] + b"\nread_1_%d-%d\n" % (st + 1, en)
    assert block in err
    assert b"\nread_13\n" in err and b"        bad ranges = 0-%d\n" % len(made["reads"][13][1]) in err  # nothing left


def test_keep_percent_over_the_children(made):
    want = made["want"]
    e = want.entries()
    p = _oracle.make_params(window_size=250)
    sc = [_oracle.score_read(None, q, p) for _, _, q, _ in e]
    passed = np.array([s["passed"] if ok else 0 for s, (_, _, _, ok) in zip(sc, e)], dtype=np.uint8)
    total = sum(len(s) for _, s, _ in made["reads"])
    r = _oracle.rank_and_cut(np.array([s["mean_q"] for s in sc]), np.array([s["window_q"] for s in sc]), np.array([len(s) for _, s, _, _ in e], dtype=np.int32),
                             passed, keep_percent=60.0, total_bases=total)
    expect = fastq_bytes([x[:3] for x, keep in zip(e, r["passed"]) if keep])
    rc, out, err = run(["--trim_adapters", made["fa"], "--keep_percent", "60", made["fastq"]])
    assert rc == 0 and out == expect and 0 < out.count(b"\n+\n") < len(e)
    assert b"  target: %d bp\n" % r["target_bases"] in err
    rc, out2, _ = run(["--trim_adapters", made["fa"], "--keep_percent", "60", "--gpus", "2", made["fastq"]], shim_env())
    assert rc == 0 and out2 == expect


def test_the_same_reads_by_every_road(made):
    want = made["want"]
    expect = want.stdout()
    args = ["--trim_adapters", made["fa"]]
    rc, out, err = run(args + [made["gz"]], {"FLX_CLI_BLOCK_BYTES": "20000", "FLX_CLI_CHUNK_BYTES": "30000"})  # streamed, many chunks
    assert rc == 0 and out == expect and want.after_line() in err
    rc, out, err = run(args + [made["bam"]])
    assert rc == 0 and out == want.stdout(upper=True) != expect and want.after_line() in err
    rc, out, err = run(args + ["--gzip", made["fastq"]])
    assert rc == 0 and gzip.decompress(out) == expect
    for source in (made["bam"], made["fastq"]):  # a child is encoded from text: keep_bam is off under the flag
        rc, out, err = run(args + ["--bam", source])
        assert rc == 0
        data, info = _bgzf.validate(out)
        recs, end = _bam.walk_model(data)
        assert info["eof"] and end == _bam.END and _bam.expected_fastq(recs)[0] == want.stdout(upper=True)
    rc, out, err = run(args + ["--gpus", "2", made["fastq"]], shim_env())
    assert rc == 0 and out == expect and want.after_line() in err
    rc, out, err = run(args + ["--gpus", "2", "--verbose", made["fastq"]], shim_env())
    assert rc == 0 and out == expect and re.findall(rb"^          adapters = [^\n]*\n", err, re.M) == want.verbose_lines()


def test_with_exclude(made, tmp_path):
    """the screen looks at the whole parent: a contaminant that is read_1's body takes read_1's child with it, and nothing else"""
    fa = tmp_path / "x.fa"
    fa.write_bytes(b">x\n" + made["reads"][1][1][100:-60] + b"\n")  # (its body: no adapter in the contaminant)
    rc, out, err = run(["--trim_adapters", made["fa"], "--exclude", str(fa), made["fastq"]])
    want = b"".join(b"@" + n + b"\n" + s + b"\n+\n" + q + b"\n" for n, s, q, ok in made["want"].entries() if ok and not n.startswith(b"read_1_"))
    assert rc == 0 and out == want and out != made["want"].stdout() and b"  excluded by reference: 1 reads" in err


def test_report(made, tmp_path):
    from filtlong_amd import api
    rep = tmp_path / "r.json"
    rc, out, err = run(["--trim_adapters", made["fa"], "--report", str(rep), made["fastq"]])
    assert rc == 0
    got = json.loads(rep.read_bytes())
    e = made["want"].entries()
    p = _oracle.make_params(window_size=250)
    sc = [_oracle.score_read(None, q, p) for _, _, q, _ in e]
    ctx = api.Context(0)
    try:
        scored = ctx.summary([len(s) for _, s, _, _ in e], [s["mean_q"] for s in sc], [s["window_q"] for s in sc])
    finally:
        ctx.close()
    assert got["scored"] == scored and got["scored"]["n"] == len(e) and got["input"]["n"] == 60
    assert got["kept"]["n"] == sum(1 for x in e if x[3] and len(x[1]) >= 1)
