"""--split_adapters through the whole command line, against tests/_adapters_split_model.py: stdout holds the model's children, named
name_start-end, and the untouched reads whole; a read of which nothing is left is gone; the "split at adapters" and "after adapter
trimming" lines, the --verbose lines and --report's scored count are the model's; a streamed gzip input, a BAM input, --gzip, --bam
and --gpus 2 give the same reads; with --trim_adapters alone the output is the ends rule's (tests/_adapters_model.py), and without
any flag every read comes out whole."""
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
import _adapters_split_model as split
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
    """split_errors None: the ends rule alone (--trim_adapters without --split_adapters)"""

    def __init__(self, reads, split_errors=10):
        self.reads = reads
        pats = model.patterns(SEQS)
        self.rows = []
        for _, s, _ in reads:
            if split_errors is None:
                kh, kt = model.end_key(s, 0, WINDOW, pats, ERRORS), model.end_key(s, 1, WINDOW, pats, ERRORS)
                ch, first, last = model.child_of(len(s), kh, kt)
            else:
                kh, kt, _, ch, first, last = split.split_of(s, WINDOW, pats, ERRORS, split_errors)
            self.rows.append((kh, kt, ch, first, last))

    def entries(self):
        out = []
        for (n, s, q), (kh, kt, ch, first, last) in zip(self.reads, self.rows):
            if not ch:
                out.append((n, s, q, first != -1))
            for st, en in ch:
                out.append((n + b"_%d-%d" % (st + 1, en), s[st:en], q[st:en], True))
        return out

    def stdout(self, min_length=1, upper=False):
        return fastq_bytes([(n, s.upper() if upper else s, q) for n, s, q, ok in self.entries() if ok and len(s) >= min_length])

    def lines(self):
        e = self.entries()
        return (b"  split at adapters: %d reads\n" % sum(len(r[2]) >= 2 for r in self.rows)
                + b"  after adapter trimming: %d reads (%d bp)\n" % (len(e), sum(len(s) for _, s, _, _ in e)))

    def middle_lines(self):
        """the maximal runs of marked bases inside [s, e): what the children leave of it"""
        out = []
        for (_, s, _), (kh, kt, ch, first, last) in zip(self.reads, self.rows):
            lo, hi = int(kh) >> 8, len(s) - (int(kt) >> 8)
            gaps = []
            if ch:
                at = lo
                for st, en in ch:
                    if st > at:
                        gaps.append(st - at)
                    at = en
                if at < hi:
                    gaps.append(hi - at)
            elif first == -1 and lo < hi:
                gaps.append(hi - lo)
            out.append(b"          middle adapters = %d ranges (%d bp)\n" % (len(gaps), sum(gaps)))
        return out


@pytest.fixture(scope="module")
def made(tmp_path_factory):
    """48 reads: chimeras of two and three parts, adapters at the ends, both, neither; one read that is all adapter"""
    d = tmp_path_factory.mktemp("adapters_split_cli")
    rng = np.random.default_rng(616)
    reads = []
    for i in range(48):
        body = lambda: cases.random_seq(rng, int(rng.integers(300, 1400)))
        a = SEQS[i % 2]
        seq = body()
        if i % 3 == 0:
            seq += (cases.substitute(rng, a, 2) if i % 2 else a) + body()
        if i % 12 == 6:
            seq += model.revcomp(SEQS[1]) + body()
        if i % 4 == 1:
            seq = cases.random_seq(rng, 5) + a + seq
        if i % 4 == 2:
            seq += model.revcomp(a) + cases.random_seq(rng, 7)
        if i == 13:
            seq = SEQS[0] + model.revcomp(SEQS[1]) + SEQS[1]
        if i == 15:
            seq = seq.lower()
        reads.append((b"read_%d" % i, seq, synth.qual_read(5000 + i, len(seq)).tobytes()))
    fa = b"".join(b">" + n + b" a comment\n" + s + b"\n" for n, s in zip(NAMES, SEQS))
    (d / "adapters.fa").write_bytes(fa)
    (d / "made.fastq").write_bytes(fastq_bytes(reads))
    (d / "made.fastq.gz").write_bytes(gzip.compress(fastq_bytes(reads)))
    (d / "made.bam").write_bytes(gen_bam.bgzf(gen_bam.fastq_to_bam(fastq_bytes(reads))))
    want = Expected(reads)
    counts = [len(r[2]) for r in want.rows]
    assert sum(c == 2 for c in counts) >= 10 and sum(c == 3 for c in counts) >= 2 and sum(c == 1 for c in counts) >= 8 and sum(c == 0 for c in counts) >= 8
    assert any(not ok for _, _, _, ok in want.entries())
    return {"dir": d, "reads": reads, "fa": str(d / "adapters.fa"), "fastq": str(d / "made.fastq"), "gz": str(d / "made.fastq.gz"),
            "bam": str(d / "made.bam"), "want": want}


def test_stdout_is_the_children(made):
    want = made["want"]
    args = ["--trim_adapters", made["fa"], "--split_adapters"]
    rc, out, err = run(args + [made["fastq"]])
    assert rc == 0 and b"Error" not in err, err[-2000:]
    assert out == want.stdout()
    assert want.lines() in err
    rc, out2, _ = run(args + ["--min_length", "600", made["fastq"]])  # the children are judged as reads of their own
    assert rc == 0 and out2 == want.stdout(min_length=600) and out2 != out
    strict = Expected(made["reads"], split_errors=0)  # --adapter_split_errors reaches the kernel
    rc, out3, err3 = run(args + ["--adapter_split_errors", "0", made["fastq"]])
    assert rc == 0 and out3 == strict.stdout() and out3 != out and strict.lines() in err3


def test_trim_adapters_alone_and_no_flag(made):
    ends = Expected(made["reads"], split_errors=None)
    rc, out, err = run(["--trim_adapters", made["fa"], made["fastq"]])
    e = ends.entries()
    assert rc == 0 and out == ends.stdout() and out != made["want"].stdout()
    assert b"  after adapter trimming: %d reads (%d bp)\n" % (len(e), sum(len(s) for _, s, _, _ in e)) in err
    assert b"split at adapters" not in err
    rc, _, verr = run(["--trim_adapters", made["fa"], "--verbose", made["fastq"]])
    assert rc == 0 and b"middle adapters" not in verr and verr.count(b"          adapters = ") == len(made["reads"])
    rc, out, err = run(["--min_length", "1", made["fastq"]])
    assert rc == 0 and out == fastq_bytes(made["reads"]) and b"adapter" not in err.lower() and b"after" not in err


def test_verbose_lines(made):
    want = made["want"]
    rc, out, err = run(["--trim_adapters", made["fa"], "--split_adapters", "--verbose", made["fastq"]])
    assert rc == 0 and out == want.stdout()
    assert re.findall(rb"^          middle adapters = [^\n]*\n", err, re.M) == want.middle_lines()
    assert re.search(rb"^          adapters = [^\n]*\n          middle adapters = ", err, re.M)  # behind the adapters' line
    kh, kt, ch, first, last = want.rows[0]
    assert len(ch) == 2 and b"      child ranges = %d-%d, %d-%d\n" % (ch[0][0], ch[0][1], ch[1][0], ch[1][1]) in err


def test_the_same_reads_by_every_road(made):
    want = made["want"]
    expect = want.stdout()
    args = ["--trim_adapters", made["fa"], "--split_adapters"]
    rc, out, err = run(args + [made["gz"]], {"FLX_CLI_BLOCK_BYTES": "20000", "FLX_CLI_CHUNK_BYTES": "30000"})  # streamed, many chunks
    assert rc == 0 and out == expect and want.lines() in err
    rc, out, err = run(args + [made["bam"]])
    assert rc == 0 and out == want.stdout(upper=True) != expect and want.lines() in err
    rc, out, err = run(args + ["--gzip", made["fastq"]])
    assert rc == 0 and gzip.decompress(out) == expect
    for source in (made["bam"], made["fastq"]):  # a child is encoded from text
        rc, out, err = run(args + ["--bam", source])
        assert rc == 0
        data, info = _bgzf.validate(out)
        recs, end = _bam.walk_model(data)
        assert info["eof"] and end == _bam.END and _bam.expected_fastq(recs)[0] == want.stdout(upper=True)
    rc, out, err = run(args + ["--gpus", "2", made["fastq"]], shim_env())
    assert rc == 0 and out == expect and want.lines() in err
    rc, out, err = run(args + ["--gpus", "2", "--verbose", made["fastq"]], shim_env())
    assert rc == 0 and out == expect and re.findall(rb"^          middle adapters = [^\n]*\n", err, re.M) == want.middle_lines()


def test_with_exclude_and_report(made, tmp_path):
    """the screen looks at the whole parent: a contaminant that is read_0's first part takes both of read_0's children with it"""
    fa = tmp_path / "x.fa"
    first = made["want"].rows[0][2][0]
    fa.write_bytes(b">x\n" + made["reads"][0][1][first[0] + 20:first[1] - 20] + b"\n")
    rep = tmp_path / "r.json"
    rc, out, err = run(["--trim_adapters", made["fa"], "--split_adapters", "--exclude", str(fa), "--report", str(rep), made["fastq"]])
    e = made["want"].entries()
    want = fastq_bytes([(n, s, q) for n, s, q, ok in e if ok and not n.startswith(b"read_0_")])
    assert rc == 0 and out == want and out != made["want"].stdout() and b"  excluded by reference: 1 reads" in err
    got = json.loads(rep.read_bytes())
    assert got["scored"]["n"] == len(e) and got["input"]["n"] == len(made["reads"])
