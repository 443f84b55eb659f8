"""--adapter_overhang through the whole command line, against tests/_adapters_overhang_model.py: with 8, the reads that begin or end
inside an adapter come out as name_start-end children at the model's coordinates and stderr names the overhang; without the flag and
with 0, stdout and stderr are those of --trim_adapters alone (the ends rule of tests/_adapters_model.py); --gpus 2, --gzip, --bam
and a BAM input give the same reads."""
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

import _adapters_cases as cases
import _adapters_model as plain_model
import _adapters_overhang_model as model
import _bam
import _bgzf
from filtlong_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "filtlong_amd", "bin", "filtlong")
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_bam  # noqa: E402  (the BAM writer of tools/gen_bam.py)

NAMES = [b"ligation_top", b"second"]
SEQS = [cases.LIGATION, b"GGTTGTTTCTGTTGGTGCTGATATTGC"]
WINDOW, ERRORS = 150, 20
OVERHANG_LINE = b"  overhang: up to 8 bases\n"


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
    def __init__(self, reads, overhang):
        self.reads = reads
        pats = model.patterns(SEQS)
        self.keys = model.keys_of([s for _, s, _ in reads], WINDOW, pats, ERRORS, overhang)
        self.rows = [model.child_of(len(s), k[0], k[1]) for (_, s, _), k in zip(reads, self.keys)]

    def entries(self):
        out = []
        for (n, s, q), (ch, first, last) in zip(self.reads, self.rows):
            if not ch:
                out.append((n, s, q, first != -1))
            for st, en in ch:
                out.append((n + b"_%d-%d" % (st + 1, en), s[st:en], q[st:en], True))
        return out

    def stdout(self, upper=False):
        return fastq_bytes([(n, s.upper() if upper else s, q) for n, s, q, ok in self.entries() if ok and len(s) >= 1])

    def line(self):
        e = self.entries()
        return b"  after adapter trimming: %d reads (%d bp)\n" % (len(e), sum(len(s) for _, s, _, _ in e))


@pytest.fixture(scope="module")
def made(tmp_path_factory):
    """40 reads: remnants of 20 to 22 adapter bases at the head, the tail or both; whole adapters; nothing; one read that is all remnant"""
    d = tmp_path_factory.mktemp("adapters_overhang_cli")
    rng = np.random.default_rng(515)
    reads = []
    for i in range(40):
        a = SEQS[i % 2]
        x = 6 + i % 3
        seq = cases.random_seq(rng, int(rng.integers(300, 1400)))
        if i % 4 in (0, 1):
            seq = a[x:] + seq
        if i % 4 in (1, 2):
            seq = seq + model.revcomp(a)[:len(a) - x]
        if i % 8 == 3:
            seq = cases.random_seq(rng, 5) + a + seq
        if i == 13:
            seq = SEQS[0][8:] + model.revcomp(SEQS[0])[:20]
        if i == 16:
            seq = seq.lower()
        reads.append((b"read_%d" % i, seq, synth.qual_read(6000 + i, len(seq)).tobytes()))
    fa = b"".join(b">" + n + b" a comment\n" + s + b"\n" for n, s in zip(NAMES, SEQS))
    (d / "adapters.fa").write_bytes(fa)
    (d / "made.fastq").write_bytes(fastq_bytes(reads))
    (d / "made.fastq.gz").write_bytes(gzip.compress(fastq_bytes(reads)))
    (d / "made.bam").write_bytes(gen_bam.bgzf(gen_bam.fastq_to_bam(fastq_bytes(reads))))
    want, without = Expected(reads, 8), Expected(reads, 0)
    assert (without.keys == plain_model.keys_of([s for _, s, _ in reads], WINDOW, model.patterns(SEQS), ERRORS)).all()
    assert (want.keys > without.keys).sum() >= 25 and any(first == -1 for _, first, _ in want.rows) and want.stdout() != without.stdout()
    return {"dir": d, "reads": reads, "fa": str(d / "adapters.fa"), "fastq": str(d / "made.fastq"), "gz": str(d / "made.fastq.gz"),
            "bam": str(d / "made.bam"), "want": want, "without": without}


def test_without_the_flag_and_with_zero(made):
    """both are --trim_adapters as it was: the ends rule's children, not a word about an overhang"""
    base = ["--trim_adapters", made["fa"]]
    rc0, out0, err0 = run(base + [made["fastq"]])
    rc1, out1, err1 = run(base + ["--adapter_overhang", "0", made["fastq"]])
    assert rc0 == 0 and rc1 == 0 and out0 == out1 and err0 == err1
    assert out0 == made["without"].stdout() and made["without"].line() in err0 and b"overhang:" not in err0  # (the line; the fixture's directory has the word in its name)
    assert b"Reading adapters\n  " + made["fa"].encode() + b"\n  2 sequences\n\n" in err0
    rc0, out0, err0 = run(base + ["--verbose", made["fastq"]])
    rc1, out1, err1 = run(base + ["--verbose", "--adapter_overhang", "0", made["fastq"]])
    assert rc0 == 0 and rc1 == 0 and out0 == out1 and err0 == err1


def test_children_at_the_models_coordinates(made):
    want = made["want"]
    rc, out, err = run(["--trim_adapters", made["fa"], "--adapter_overhang", "8", made["fastq"]])
    assert rc == 0 and b"Error" not in err, err[-2000:]
    assert out == want.stdout() and want.line() in err
    assert b"Reading adapters\n  " + made["fa"].encode() + b"\n  2 sequences\n" + OVERHANG_LINE + b"\n" in err
    (ch, _, _), (n, s, q) = want.rows[0], made["reads"][0]  # read_0 begins with ligation_top[6:]: 22 bases go
    assert ch == [(22, len(s))] and b"@read_0_23-%d\n" % len(s) + s[22:] + b"\n" in out
    rc, _, verr = run(["--trim_adapters", made["fa"], "--adapter_overhang", "8", "--verbose", made["fastq"]])
    assert rc == 0 and b"          adapters = start 22 (ligation_top), end 0 (none)\n" in verr
    assert verr.count(b"          adapters = ") == len(made["reads"])


def test_the_same_reads_by_every_road(made):
    want = made["want"]
    expect = want.stdout()
    args = ["--trim_adapters", made["fa"], "--adapter_overhang", "8"]
    rc, out, err = run(args + [made["gz"]], {"FLX_CLI_BLOCK_BYTES": "20000", "FLX_CLI_CHUNK_BYTES": "30000"})  # streamed, many chunks
    assert rc == 0 and out == expect and want.line() in err
    rc, out, err = run(args + [made["bam"]])
    assert rc == 0 and out == want.stdout(upper=True) != expect and want.line() in err and OVERHANG_LINE in err
    rc, out, err = run(args + ["--gzip", made["fastq"]])
    assert rc == 0 and gzip.decompress(out) == expect
    rc, out, err = run(args + ["--bam", made["fastq"]])
    assert rc == 0
    data, info = _bgzf.validate(out)
    recs, end = _bam.walk_model(data)
    assert info["eof"] and end == _bam.END and _bam.expected_fastq(recs)[0] == want.stdout(upper=True)
    rc, out, err = run(args + ["--gpus", "2", made["fastq"]], shim_env())
    assert rc == 0 and out == expect and want.line() in err
