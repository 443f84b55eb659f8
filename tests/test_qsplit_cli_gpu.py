"""--split_window_q through the whole command line, against the model of tests/_qsplit_model.py: stdout holds exactly the children's
substrings, named name_start-end like the children of --split, and the untouched reads whole; a wholly bad read is gone; the
"after splitting" line, the --verbose blocks and --report's scored summary are the model's; the reference binary, fed the children as
reads of their own, prints their blocks' numbers; and --gzip, a streamed gzip input, --gpus 2, a BAM input and --bam give the same
reads.  With --target_bases / --keep_percent the kept reads and the cut's report are those of the oracle's rank_and_cut over the
model's children and the whole reads together, by the same roads."""
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
import _qsplit_model as model

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "filtlong_amd", "bin", "filtlong")
SORT_FASTQ = os.path.join(ROOT, "tests", "golden", "ref_fixtures", "test_sort.fastq")
PHRED = dict(good=(25, 40), junk=(0, 3))
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


def made_reads():
    """60 reads: untouched ones, reads with one or two junk stretches, wholly bad ones, a read shorter than the window."""
    rng = np.random.default_rng(606)
    reads = []
    for i in range(60):
        length = int(rng.integers(300, 4000)) if i != 7 else 120
        k = (0, 1, 2, 1)[i % 4]
        st = [(int(a), int(a) + int(rng.integers(40, 400))) for a in rng.integers(0, length, size=k)]
        if i % 15 == 4:
            st = [(0, length)]
        seq = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=length).tobytes()
        reads.append((b"read_%d" % i, seq, model.junk_read(rng, length, st, **PHRED)))
    return reads


def fastq_bytes(reads):
    return b"".join(b"@" + n + b"\n" + s + b"\n+\n" + q + b"\n" for n, s, q in reads)


class Expected:
    """What the model says a run over `reads` with --window_size w --split_window_q q prints."""

    def __init__(self, reads, w, q):
        self.reads, self.w, self.q = reads, w, q
        self.off, self.rng, self.first, self.last, self.wholly = model.split_batch([r[2] for r in reads], w, q)
        self.census = model.census(self.off, self.wholly)
        assert min(self.census) > 0, self.census  # reads that split, wholly bad reads, untouched reads: all three are in the input

    def entries(self):
        """reads2: (name, seq, qual) of every child in place of its parent; a wholly bad read stays (and fails)"""
        out = []
        for i, (n, s, q) in enumerate(self.reads):
            a, b = int(self.off[i]), int(self.off[i + 1])
            if a == b:
                out.append((n, s, q, not self.wholly[i]))
            for st, en in self.rng[a:b]:
                out.append((n + b"_%d-%d" % (st + 1, en), s[st:en], q[st:en], True))
        return out

    def stdout(self, min_length=1):
        return fastq_bytes([(n, s, q) for n, s, q, ok in self.entries() if ok and len(s) >= min_length])

    def after_splitting(self):
        e = self.entries()
        return b"  after splitting: %d reads (%d bp)\n" % (len(e), sum(len(s) for _, s, _, _ in e))

    def reads2_bases(self):
        return sum(len(s) for _, s, _, _ in self.entries())

    def filtered(self, target_bases=None, keep_percent=None, min_length=None, lw=1.0):
        """(stdout, [the "target:" line, the line behind it]) of a run with --target_bases / --keep_percent: every reads2 entry
        scored by the oracle as a read of its own (a wholly bad read fails, and still counts in the statistics), the oracle's
        rank_and_cut with total_bases the INPUT's bases."""
        e = self.entries()
        p = _oracle.make_params(window_size=self.w, min_length=min_length)
        sc = [_oracle.score_read(None, q, p) for _, _, q, _ in e]
        passed = np.array([s["passed"] if ok else 0 for s, (_, _, _, ok) in zip(sc, e)], dtype=np.uint8)
        r = _oracle.rank_and_cut(np.array([s["mean_q"] for s in sc]), np.array([s["window_q"] for s in sc]),
                                 np.array([len(s) for _, s, _, _ in e], dtype=np.int32), passed, lw=lw, target_bases=target_bases,
                                 keep_percent=keep_percent, total_bases=sum(len(s) for _, s, _ in self.reads))
        second = {1: b"  not enough reads to reach target\n", 2: b"  reads already fall below target after filtering\n",
                  3: b"  keeping %d bp\n" % r["kept_bases"]}[r["outcome"]]
        return fastq_bytes([x[:3] for x, keep in zip(e, r["passed"]) if keep]), [b"  target: %d bp\n" % r["target_bases"], second]


def cut_lines(err):
    """The "target:" line of a run's stderr and the line behind it."""
    lines = err.split(b"\n")
    at = [k for k, l in enumerate(lines) if l.startswith(b"  target: ")]
    assert len(at) == 1, err[-2000:]
    return [lines[at[0]] + b"\n", lines[at[0] + 1] + b"\n"]


@pytest.fixture(scope="module")
def made(tmp_path_factory):
    d = tmp_path_factory.mktemp("qsplit_cli")
    reads = made_reads()
    (d / "made.fastq").write_bytes(fastq_bytes(reads))
    (d / "made.fastq.gz").write_bytes(gzip.compress(fastq_bytes(reads)))
    (d / "made.bam").write_bytes(gen_bam.bgzf(gen_bam.fastq_to_bam(fastq_bytes(reads))))
    recs = [_bam.rec(n, s.decode(), bytes(c - 33 for c in q), tags=b"RGZg1\0") for n, s, q in reads]  # ... and one with tags
    (d / "tags.bam").write_bytes(_bam.bgzf(_bam.bam_bytes(recs, text=b"@HD\tVN:1.6\tSO:unsorted\n")))
    return {"dir": d, "reads": reads, "fastq": str(d / "made.fastq"), "gz": str(d / "made.fastq.gz"), "bam": str(d / "made.bam"),
            "tags_bam": str(d / "tags.bam"), "want": Expected(reads, 250, 85)}


ARGS = ["--window_size", "250", "--split_window_q", "85"]


def test_stdout_is_the_children(made):
    want = made["want"]
    rc, out, err = run(ARGS + [made["fastq"]])
    assert rc == 0 and out == want.stdout()
    assert want.after_splitting() in err and b"Error" not in err
    # with a hard cut-off the children are judged as reads of their own
    rc, out, err = run(ARGS + ["--min_length", "500", made["fastq"]])
    assert rc == 0 and out == want.stdout(min_length=500) and out != want.stdout()
    # without the flag the reads come out whole and nothing speaks of splitting
    rc, out, err = run(["--min_length", "1", made["fastq"]])
    assert rc == 0 and out == fastq_bytes(made["reads"]) and b"after splitting" not in err


def test_the_fixture_of_the_reference(tmp_path):
    reads = [(n.encode(), s, q) for n, s, q in _oracle.read_fastx(SORT_FASTQ)]
    want = Expected(reads, 10, 97)  # one read splits into 14 children, one is wholly bad, one stays whole
    rc, out, err = run(["--window_size", "10", "--split_window_q", "97", SORT_FASTQ])
    assert rc == 0 and out == want.stdout() and want.after_splitting() in err


def verbose_blocks(err):
    """{name: (length, mean quality, window quality)} and the bad / child range lines of a --verbose run's stderr"""
    text = err.decode()
    blocks = {m.group(1): (int(m.group(2)), m.group(3), m.group(4))
              for m in re.finditer(r"\n(\S+)\n +length = (\d+) +mean quality = (\S+) +window quality = (\S+)\n", text)}
    bad = re.findall(r"\n(\S+)\n +length = [^\n]*\n +bad ranges = ([^\n]*)\n", text)
    kids = re.findall(r" +child ranges = ([^\n]*)\n", text)
    return blocks, dict(bad), kids


def test_verbose_and_report_and_the_reference(made, tmp_path):
    want = made["want"]
    rep = tmp_path / "report.json"
    rc, out, err = run(ARGS + ["--verbose", "--report", str(rep), made["fastq"]])
    assert rc == 0 and out == want.stdout() and want.after_splitting() in err
    blocks, bad, kids = verbose_blocks(err)
    entries = want.entries()
    n_children = 0
    for i, (n, s, q) in enumerate(made["reads"]):
        a, b = int(want.off[i]), int(want.off[i + 1])
        name = n.decode()
        assert blocks[name][0] == len(s)
        if want.wholly[i]:
            assert bad[name] == "0-%d" % len(s)
        elif a == b:
            assert name not in bad
        else:
            gaps, at = [], 0
            for st, en in want.rng[a:b]:
                if st > at:
                    gaps.append("%d-%d" % (at, st))
                at = en
            if at < len(s):
                gaps.append("%d-%d" % (at, len(s)))
            assert bad[name] == ", ".join(gaps)
            assert ", ".join("%d-%d" % (st, en) for st, en in want.rng[a:b]) in kids
            n_children += b - a
    assert len(kids) == int((np.diff(want.off.astype(np.int64)) > 0).sum()) and n_children == len(want.rng)
    for n, s, q, ok in entries:
        assert blocks[n.decode()][0] == len(s)
    # --report: the scored reads are reads2
    scored = json.loads(rep.read_bytes())["scored"]
    assert scored["n"] == len(entries) and scored["bases"] == sum(len(s) for _, s, _, _ in entries)
    # the reference binary over the children as reads of their own prints the numbers of our child blocks
    if not _oracle.have_ref():
        pytest.fail("oracle/_ref is not built: build() makes the reference binary")
    children = [(n, s, q) for i, (n, s, q, ok) in enumerate(entries) if b"_" in n[5:]]
    assert len(children) == len(want.rng)
    path = tmp_path / "children.fastq"
    path.write_bytes(fastq_bytes(children))
    rrc, rout, rerr = _oracle.run_ref_filtlong(["--min_length", "1", "--window_size", "250", "--verbose", str(path)])
    assert rrc == 0
    ref_blocks, _, _ = verbose_blocks(rerr.encode())
    for n, s, q in children:
        assert ref_blocks[n.decode()] == blocks[n.decode()], n


def test_the_same_bytes_by_every_road(made):
    want = made["want"].stdout()
    rc, out, err = run(ARGS + ["--gzip", made["fastq"]])
    assert rc == 0 and gzip.decompress(out) == want
    # a gzip input forced through the streamed path, in many small blocks and chunks
    rc, out, err = run(ARGS + [made["gz"]], {"FLX_CLI_BLOCK_BYTES": "20000", "FLX_CLI_CHUNK_BYTES": "30000"})
    assert rc == 0 and out == want and made["want"].after_splitting() in err
    rc, out, err2 = run(ARGS + ["--gpus", "2", made["fastq"]], shim_env())
    assert rc == 0 and out == want and made["want"].after_splitting() in err2
    # a BAM input: children are encoded from text
    rc, out, err = run(ARGS + [made["bam"]])
    assert rc == 0 and out == want


def test_bam_out_is_the_children_without_tags(made):
    for path in (made["fastq"], made["bam"], made["tags_bam"]):
        rc, out, err = run(ARGS + ["--bam", path])
        assert rc == 0
        data, info = _bgzf.validate(out)
        assert info["eof"]
        records, end = _bam.walk_model(data)
        assert end == _bam.END and _bam.expected_fastq(records)[0] == made["want"].stdout()
        assert b"RGZ" not in data and all(r["flag"] == 4 for r in records)


def filtered_run(want, args, path, extra=None, **kw):
    """One run with a cut: stdout and the two lines of the cut's report are the oracle's over the model's children."""
    out_want, lines_want = want.filtered(**kw)
    rc, out, err = run(ARGS + args + [path], extra)
    assert rc == 0 and b"Error" not in err, err[-2000:]
    assert cut_lines(err) == lines_want and want.after_splitting() in err
    assert out == out_want, "stdout differs: %d bytes, %d expected" % (len(out), len(out_want))
    return out_want, lines_want


def test_target_bases_and_keep_percent_over_the_children(made):
    """The global stage behind the split: the cut ranks children and whole reads together, a wholly bad read counts in the quality
    statistics and the percentage is of the input's bases, not of what is left after splitting."""
    want = made["want"]
    b2 = want.reads2_bases()
    outs = []
    for t in (b2 // 3, 2 * b2 // 3):
        out, lines = filtered_run(want, ["--target_bases", str(t)], made["fastq"], target_bases=t)
        assert lines[0] == b"  target: %d bp\n" % t and lines[1].startswith(b"  keeping ")
        outs.append(out)
    assert 0 < len(outs[0]) < len(outs[1]) < len(want.stdout())
    assert re.search(rb"^@read_\d+_\d+-\d+$", outs[0], re.M), "no child among the kept reads"
    out, lines = filtered_run(want, ["--keep_percent", "60"], made["fastq"], keep_percent=60.0)
    total = sum(len(s) for _, s, _ in made["reads"])
    assert lines[0] == b"  target: %d bp\n" % int(0.6 * total) and b2 < total
    t = b2 // 2
    out, _ = filtered_run(want, ["--target_bases", str(t), "--min_length", "500", "--length_weight", "0"], made["fastq"],
                          target_bases=t, min_length=500, lw=0.0)
    assert 0 < len(out) < len(want.stdout(min_length=500))
    # more than reads2 holds, less than the input: the reads "already fall below", they are not "not enough"
    _, lines = filtered_run(want, ["--target_bases", str(b2 + 1)], made["fastq"], target_bases=b2 + 1)
    assert lines[1] == b"  reads already fall below target after filtering\n" and b2 + 1 < total


def test_the_cut_by_every_road(made):
    want = made["want"]
    t = want.reads2_bases() // 3
    filtered_run(want, ["--target_bases", str(t), "--gpus", "2"], made["fastq"], shim_env(), target_bases=t)
    filtered_run(want, ["--keep_percent", "60"], made["gz"], {"FLX_CLI_BLOCK_BYTES": "20000", "FLX_CLI_CHUNK_BYTES": "30000"}, keep_percent=60.0)
    out_want, lines_want = want.filtered(target_bases=t)
    rc, out, err = run(ARGS + ["--target_bases", str(t), "--bam", made["fastq"]])
    assert rc == 0 and cut_lines(err) == lines_want
    data, info = _bgzf.validate(out)
    records, end = _bam.walk_model(data)
    assert info["eof"] and end == _bam.END and _bam.expected_fastq(records)[0] == out_want
