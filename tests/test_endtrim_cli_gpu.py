"""--trim_ends_q through the whole command line, against tests/_endtrim_model.py: stdout holds the model's trimmed records, named
name_start-end like every child, and the untouched reads whole; a read of which nothing is left is gone; the "after quality trimming"
line, the --verbose lines and --report's scored summary are the model's; a streamed gzip input, a BAM input, --gzip, --bam and --gpus 2
give the same reads; --exclude and --max_low_complexity look at the whole parent; a FASTA input is refused as under --split_window_q;
without the flag every byte of stdout, stderr and the report is what the reference binary's golden records say."""
import gzip
import hashlib
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import _bam
import _bgzf
import _cases
import _endtrim_cases as cases
import _endtrim_model as model
import _oracle
import _summary

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "filtlong_amd", "bin", "filtlong")
FIX = _cases.FIXTURES
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_bam  # noqa: E402  (the BAM writer of tools/gen_bam.py)

Q = "90"


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
    def __init__(self, reads):
        from filtlong_amd import api
        self.reads = reads
        self.cuts = model.batch_cuts([q for _, _, q in reads], api.qsplit_threshold(float(Q)))

    def entries(self):
        """reads2: (name, seq, qual, may pass) — the child in place of its parent; a read of which nothing is left stays and fails"""
        out = []
        for (n, s, q), (h, c) in zip(self.reads, self.cuts):
            k, first, last = model.child_of(int(h), int(c), len(s))
            if k:
                out.append((n + b"_%d-%d" % (first + 1, last), s[first:last], q[first:last], True))
            else:
                out.append((n, s, q, first != -1))
        return out

    def stdout(self, min_length=1):
        return fastq_bytes([(n, s, q) for n, s, q, ok in self.entries() if ok and len(s) >= min_length])

    def after_line(self):
        e = self.entries()
        return b"  after quality trimming: %d reads (%d bp)\n" % (len(e), sum(len(s) for _, s, _, _ in e))

    def verbose_lines(self):
        return [b"          quality trim = start %d, end %d\n" % (int(h), int(c)) for h, c in self.cuts]


@pytest.fixture(scope="module")
def made(tmp_path_factory):
    """40 reads: junk at the head, the tail, both, neither; three that are wholly junk; upper-case bases, so that BAM gives them back"""
    d = tmp_path_factory.mktemp("endtrim_cli")
    rng = np.random.default_rng(616)
    reads = []
    for i in range(40):
        n = int(rng.integers(200, 1500))
        head = int(rng.integers(5, 80)) if i % 4 in (0, 1) else 0
        tail = int(rng.integers(5, 80)) if i % 4 in (1, 2) else 0
        qual = cases.ont_like(rng, n, head, tail) if i % 4 != 3 else cases.rand_bytes(rng, n, ord("?"), ord("I"))
        if i in (13, 21, 34):
            qual = cases.rand_bytes(rng, n, 33, 38)
        seq = bytes(rng.choice(list(b"ACGT"), size=n).astype(np.uint8))
        reads.append((b"read_%d" % i, seq, qual))
    (d / "made.fastq").write_bytes(fastq_bytes(reads))
    (d / "made.fastq.gz").write_bytes(gzip.compress(fastq_bytes(reads)))
    (d / "made.bam").write_bytes(gen_bam.bgzf(gen_bam.fastq_to_bam(fastq_bytes(reads))))
    (d / "made.fasta").write_bytes(b"".join(b">" + n + b"\n" + s + b"\n" for n, s, _ in reads))
    want = Expected(reads)
    cut = want.cuts
    assert (cut[:, 0] > 0).sum() >= 15 and (cut[:, 1] > 0).sum() >= 15 and ((cut[:, 0] == 0) & (cut[:, 1] == 0)).sum() >= 8
    # (the three wholly junk ones, and any read so short that the junk of one end outweighs its whole middle: both cuts are over the whole read)
    assert 3 <= sum(1 for _, _, _, ok in want.entries() if not ok) <= 8
    return {"dir": d, "reads": reads, "fastq": str(d / "made.fastq"), "gz": str(d / "made.fastq.gz"), "bam": str(d / "made.bam"),
            "fasta": str(d / "made.fasta"), "want": want}


def test_stdout_is_the_trimmed_reads(made):
    want = made["want"]
    rc, out, err = run(["--trim_ends_q", Q, made["fastq"]])
    assert rc == 0 and b"Error" not in err, err[-2000:]
    assert out == want.stdout()
    assert want.after_line() in err and err.index(b"Scoring long reads") < err.index(want.after_line())
    assert len(re.findall(rb"^@read_\d+_\d+-\d+$", out, re.M)) >= 25 and len(re.findall(rb"^@read_\d+$", out, re.M)) >= 8  # children: name_start-end
    # with a hard cut-off the children are judged as reads of their own
    rc, out2, _ = run(["--trim_ends_q", Q, "--min_length", "600", made["fastq"]])
    assert rc == 0 and out2 == want.stdout(min_length=600) and out2 != out
    # another Q reaches the kernel
    rc, out3, _ = run(["--trim_ends_q", "99", made["fastq"]])
    assert rc == 0 and out3 != out


def test_verbose_lines(made):
    want = made["want"]
    rc, out, err = run(["--trim_ends_q", Q, "--verbose", made["fastq"]])
    assert rc == 0 and out == want.stdout()
    got = re.findall(rb"^          quality trim = [^\n]*\n", err, re.M)
    assert got == want.verbose_lines()
    # the block of a trimmed read: bad ranges, child ranges, the cuts' line, then the child's own block
    (n, s, q), (h, c) = made["reads"][1], want.cuts[1]
    st, en = int(h), len(s) - int(c)
    assert st > 0 and en < len(s)
    block = b"        bad ranges = 0-%d, %d-%d\n      child ranges = %d-%d\n" % (st, en, len(s), st, en) + want.verbose_lines()[1] + b"\nread_1_%d-%d\n" % (st + 1, en)
    assert block in err
    assert b"\nread_13\n" in err and b"        bad ranges = 0-%d\n" % len(made["reads"][13][1]) in err  # nothing left
    # an untouched read: neither line, and the cuts' line says 0, 0
    assert b"\nread_3\n" in err and want.verbose_lines()[3] == b"          quality trim = start 0, end 0\n"


def test_the_same_reads_by_every_road(made):
    want = made["want"]
    expect = want.stdout()
    args = ["--trim_ends_q", Q]
    rc, out, err = run(args + [made["gz"]], {"FLX_CLI_BLOCK_BYTES": "20000", "FLX_CLI_CHUNK_BYTES": "30000"})  # streamed, many chunks
    assert rc == 0 and out == expect and want.after_line() in err
    rc, out, err = run(args + [made["bam"]])
    assert rc == 0 and out == expect and want.after_line() in err
    rc, out, err = run(args + ["--gzip", made["fastq"]])
    assert rc == 0 and gzip.decompress(out) == expect
    for source in (made["bam"], made["fastq"]):  # a child is encoded from text: keep_bam is off under the flag
        rc, out, err = run(args + ["--bam", source])
        assert rc == 0
        data, info = _bgzf.validate(out)
        recs, end = _bam.walk_model(data)
        assert info["eof"] and end == _bam.END and _bam.expected_fastq(recs)[0] == expect
    rc, out, err = run(args + ["--gpus", "2", made["fastq"]], shim_env())
    assert rc == 0 and out == expect and want.after_line() in err
    rc, out, err = run(args + ["--gpus", "2", "--verbose", made["fastq"]], shim_env())
    assert rc == 0 and out == expect and re.findall(rb"^          quality trim = [^\n]*\n", err, re.M) == want.verbose_lines()


def test_fasta_input_is_refused_as_under_split_window_q(made):
    """a FASTA read has no qualities and Phred mode cannot score it: the reference's error, with and without the flag"""
    a = run(["--split_window_q", "85", made["fasta"]])
    b = run(["--trim_ends_q", Q, made["fasta"]])
    assert a[0] == b[0] == 1 and a[1] == b[1] == b"" and b"Error: FASTA input not supported without an external reference" in b[2]


def test_with_exclude_and_low_complexity(made, tmp_path):
    """both look at the whole parent: a contaminant that is read_1 takes read_1's child with it, and nothing else"""
    fa = tmp_path / "x.fa"
    fa.write_bytes(b">x\n" + made["reads"][1][1] + b"\n")
    rc, out, err = run(["--trim_ends_q", Q, "--exclude", str(fa), "--max_low_complexity", "50", made["fastq"]])
    want = fastq_bytes([(n, s, q) for n, s, q, ok in made["want"].entries() if ok and not n.startswith(b"read_1_")])
    assert rc == 0 and out == want and out != made["want"].stdout()
    assert b"  excluded by reference: 1 reads" in err and b"  low complexity: 0 reads" in err


def test_report(made, tmp_path):
    from filtlong_amd import api
    rep = tmp_path / "r.json"
    rc, out, err = run(["--trim_ends_q", Q, "--report", str(rep), made["fastq"]])
    assert rc == 0 and out == made["want"].stdout()
    got = json.loads(rep.read_bytes())
    e = made["want"].entries()
    p = _oracle.make_params(window_size=250)
    sc = [_oracle.score_read(None, q, p) for _, _, q, _ in e]
    ctx = api.Context(0)
    try:
        scored = ctx.summary([len(s) for _, s, _, _ in e], [s["mean_q"] for s in sc], [s["window_q"] for s in sc])
    finally:
        ctx.close()
    assert got["scored"] == scored and got["scored"]["n"] == len(e) == 40 and got["input"]["n"] == 40
    assert got["scored"]["bases"] == sum(len(s) for _, s, _, _ in e) < got["input"]["bases"]
    assert got["kept"]["n"] == sum(1 for x in e if x[3]) <= 37


def test_without_the_flag_every_byte_is_what_it_was(tmp_path):
    """test_sort.fastq --target_bases 10000: stdout by the sha256 the reference binary left in tests/golden/e2e.json, the whole --verbose
    stderr by tests/golden/verbose.json, the report by the numpy restatement of the summary; and nothing of the feature on stderr"""
    from filtlong_amd import api
    fq = os.path.join(FIX, "test_sort.fastq")
    gold = json.load(open(os.path.join(_cases.GOLDEN, "e2e.json")))["sort|phred|10000"]
    vgold = json.load(open(os.path.join(_cases.GOLDEN, "verbose.json")))["phred|sort|t10000"]
    rep = tmp_path / "r.json"
    rc, out, err = run(gold["args"] + ["--report", str(rep), fq])
    assert rc == gold["rc"] == 0 and len(out) == gold["stdout_len"] and hashlib.sha256(out).hexdigest() == gold["stdout_sha256"]
    assert b"quality trim" not in err and b"after" not in err
    rc, vout, verr = run(vgold["args"] + [fq])
    assert rc == vgold["rc"] and vout == out and verr.decode() == vgold["stderr"]
    recs = _oracle.read_fastx(fq)
    prm = _oracle.make_params()
    sc = [_oracle.score_read(None, q, prm) for _, _, q in recs]
    edges = api.summary_q_edges()
    got = json.loads(rep.read_bytes())
    assert list(got) == ["version", "q_edges", "input", "scored", "kept"]
    want_input = _summary.reference(np.array([len(r[1]) for r in recs]), np.array([s["mean_q"] for s in sc]), np.array([s["window_q"] for s in sc]), None, edges)
    assert not _summary.diff(got["input"], want_input) and got["scored"] == got["input"]
    assert got["kept"]["bases"] == sum(len(l) for l in out.split(b"\n")[1::4])
