"""`filtlong --report FILE`: stdout, stderr and the exit status are those of the same command without the flag, and FILE holds one
JSON object — the input reads, the scored reads (children in place of their parents) and the kept reads, each as the integer
fields of flx_summary.  Held against the numpy restatement (tests/_summary.py) of the lengths in the input file, of the records
actually on stdout and of the oracle's per-read qualities; --gzip and --gpus 2 (forked ranks over the loopback communicator)
leave the same bytes in FILE; a run that fails leaves FILE empty."""
import json
import os
import subprocess

import numpy as np
import pytest

import _cases
import _oracle
import _summary

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "filtlong_amd", "bin", "filtlong")
FIX = _cases.FIXTURES
SHIM_DIR = os.path.join(ROOT, "tests", "shim")
LENGTH_FIELDS = ("n", "bases", "min_length", "max_length", "median_length", "nx", "len_count", "len_bases")
SUMMARY_KEYS = list(_summary.FIELDS)


def run(args, extra=None):
    env = dict(os.environ, LANG="C", LC_ALL="C")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    env.update(extra or {})
    p = subprocess.run([BIN] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=300)
    return p.returncode, p.stdout, p.stderr


def with_and_without(args, tmp_path, extra=None, prefix=(), tag="report"):
    """Runs the command without and with --report; everything the reference's surface shows is the same.  -> (plain run, report bytes)"""
    path = tmp_path / (tag + ".json")
    path.write_text("stale")
    plain = run(list(prefix) + args, extra)
    reported = run(list(prefix) + ["--report", str(path)] + args, extra)
    assert reported == plain, (args, reported[2][-600:], plain[2][-600:])
    return plain, path.read_bytes()


def fastq_names_and_lengths(blob):
    lines = blob.split(b"\n")
    assert lines[-1] == b"" and (len(lines) - 1) % 4 == 0
    return [l[1:].split()[0].decode() for l in lines[0:-1:4]], [len(l) for l in lines[1:-1:4]]


def parsed(blob, edges):
    rep = json.loads(blob)
    assert list(rep) == ["version", "q_edges", "input", "scored", "kept"] and rep["version"] == 1
    assert rep["q_edges"] == [float(e) for e in edges]  # (%.17g round-trips)
    for k in ("input", "scored", "kept"):
        assert list(rep[k]) == SUMMARY_KEYS
    return rep


@pytest.fixture(scope="module")
def edges():
    from filtlong_amd import api
    return api.summary_q_edges()


@pytest.fixture(scope="module")
def phred(edges):
    """test_sort.fastq through the oracle, once: names, lengths and the per-read qualities of Phred mode."""
    recs = _oracle.read_fastx(os.path.join(FIX, "test_sort.fastq"))
    prm = _oracle.make_params()
    sc = [_oracle.score_read(None, q, prm) for _, _, q in recs]
    return {"names": [r[0] for r in recs], "length": np.array([len(r[1]) for r in recs]),
            "mean": np.array([s["mean_q"] for s in sc]), "window": np.array([s["window_q"] for s in sc])}


PHRED_RUNS = [["--target_bases", "8000"], ["--keep_percent", "50"], ["--min_length", "1000"]]


@pytest.mark.parametrize("flags", PHRED_RUNS, ids=[f[0][2:] for f in PHRED_RUNS])
def test_phred_run(tmp_path, edges, phred, flags):
    args = flags + [os.path.join(FIX, "test_sort.fastq")]
    (rc, out, err), blob = with_and_without(args, tmp_path)
    assert rc == 0 and out
    rep = parsed(blob, edges)
    want_input = _summary.reference(phred["length"], phred["mean"], phred["window"], None, edges)
    assert not _summary.diff(rep["input"], want_input)
    assert rep["scored"] == rep["input"]  # no children: reads2 is the input
    names, lengths = fastq_names_and_lengths(out)
    assert 0 < len(names) <= len(phred["names"]) and len(set(phred["names"])) == len(phred["names"])
    assert len(names) < len(phred["names"]) or flags[0] == "--min_length"
    on_stdout = _summary.reference(lengths, None, None, None, edges)
    assert {k: rep["kept"][k] for k in LENGTH_FIELDS} == {k: on_stdout[k] for k in LENGTH_FIELDS}
    mask = np.isin(np.array(phred["names"]), names)
    assert not _summary.diff(rep["kept"], _summary.reference(phred["length"], phred["mean"], phred["window"], mask, edges))
    # --gzip: the same report bytes
    path = tmp_path / "gz.json"
    rcz, outz, errz = run(["--gzip", "--report", str(path)] + args)
    assert (rcz, errz) == (rc, err) and path.read_bytes() == blob


def test_kmer_run_with_children(tmp_path, edges):
    fq = os.path.join(FIX, "test_split.fastq")
    args = ["-a", os.path.join(FIX, "test_reference.fasta"), "--trim", "--split", "100", "--target_bases", "8000", fq]
    (rc, out, err), blob = with_and_without(args, tmp_path)
    assert rc == 0 and out
    rep = parsed(blob, edges)
    # the oracle's reads2 entries
    ks = _oracle.KmerSet()
    ks.add_assembly([s for _, s, _ in _oracle.read_fastx(os.path.join(FIX, "test_reference.fasta"))])
    recs = _oracle.read_fastx(fq)
    prm = _oracle.make_params(trim=True, split=100)
    from filtlong_amd import api
    plane, offsets, lengths = api.pack_reads([seq for _, seq, _ in recs])
    sc = _oracle.score_plane_mt(plane, offsets, lengths, prm, ks)
    assert not _summary.diff(rep["input"], _summary.reference(lengths, sc["mean_q"], sc["window_q"], None, edges))
    r2 = _oracle.reads2_gather(lengths, sc)  # a read with children is replaced by them, one without stays itself
    assert len(r2["length"]) > len(lengths)
    assert not _summary.diff(rep["scored"], _summary.reference(r2["length"], r2["mean_q"], r2["window_q"], None, edges))
    assert rep["scored"] != rep["input"]
    names, lengths = fastq_names_and_lengths(out)
    on_stdout = _summary.reference(lengths, None, None, None, edges)
    assert {k: rep["kept"][k] for k in LENGTH_FIELDS} == {k: on_stdout[k] for k in LENGTH_FIELDS}
    assert 0 < rep["kept"]["n"] < rep["scored"]["n"] and sum(rep["kept"]["mean_q_count"]) == rep["kept"]["n"]
    path = tmp_path / "gz.json"
    rcz, outz, errz = run(["--gzip", "--report", str(path)] + args)
    assert (rcz, errz) == (rc, err) and path.read_bytes() == blob


def test_two_ranks_leave_the_same_report(tmp_path, edges):
    subprocess.check_call(["make", "-s", "-C", SHIM_DIR])
    extra = {"FLX_RCCL_LIB": os.path.join(SHIM_DIR, "libloopback_rccl.so"), "FLX_DEVICE": "0"}
    for i, args in enumerate((["--target_bases", "8000", os.path.join(FIX, "test_sort.fastq")],
                              ["--verbose", "--keep_percent", "50", os.path.join(FIX, "test_sort.fastq")],
                              ["-a", os.path.join(FIX, "test_reference.fasta"), "--trim", "--split", "100", "--target_bases", "8000",
                               os.path.join(FIX, "test_split.fastq")])):
        (rc, out, err), one = with_and_without(args, tmp_path, tag="one%d" % i)
        (rc2, out2, err2), two = with_and_without(args, tmp_path, extra, ["--gpus", "2"], tag="two%d" % i)
        assert rc == 0 and rc2 == 0 and out2 == out
        parsed(one, edges)
        assert two == one, args
        path = tmp_path / ("two_gz%d.json" % i)
        assert run(["--gpus", "2", "--gzip", "--report", str(path)] + args, extra)[0] == 0 and path.read_bytes() == one


def test_reads_of_many_lengths_one_and_three_ranks(tmp_path, edges):
    """The fixtures hold three and four reads; here 400 of 40 .. 6000 bases, so that the histograms and the order statistics have
    something to tell apart and every rank of three holds a share."""
    from filtlong_amd import synth
    rng = np.random.RandomState(3)
    lengths = rng.randint(40, 6000, 400)
    quals = [synth.qual_read(i, int(n)).tobytes() for i, n in enumerate(lengths)]
    fq = tmp_path / "many.fastq"
    fq.write_bytes(b"".join(b"@r%d\n%s\n+\n%s\n" % (i, b"A" * len(q), q) for i, q in enumerate(quals)))
    args = ["--min_length", "500", "--keep_percent", "70", str(fq)]
    (rc, out, err), blob = with_and_without(args, tmp_path)
    assert rc == 0
    rep = parsed(blob, edges)
    prm = _oracle.make_params(min_length=500)
    sc = [_oracle.score_read(None, q, prm) for q in quals]
    mean, window = [s["mean_q"] for s in sc], [s["window_q"] for s in sc]
    assert not _summary.diff(rep["input"], _summary.reference(lengths, mean, window, None, edges))
    assert rep["scored"] == rep["input"]
    names, kept_lengths = fastq_names_and_lengths(out)
    mask = np.isin(np.array(["r%d" % i for i in range(400)]), names)
    assert 0 < mask.sum() < (lengths >= 500).sum()
    assert not _summary.diff(rep["kept"], _summary.reference(lengths, mean, window, mask, edges))
    subprocess.check_call(["make", "-s", "-C", SHIM_DIR])
    extra = {"FLX_RCCL_LIB": os.path.join(SHIM_DIR, "libloopback_rccl.so"), "FLX_DEVICE": "0"}
    (rc3, out3, err3), three = with_and_without(args, tmp_path, extra, ["--gpus", "3"], tag="three")
    assert rc3 == 0 and out3 == out and three == blob


def test_failing_run_leaves_an_empty_file(tmp_path):
    for args in (["--target_bases", "1000", os.path.join(FIX, "test_bad_fastq.fastq")],
                 ["--verbose", "--target_bases", "1000", os.path.join(FIX, "test_bad_fastq.fastq")]):
        (rc, out, err), blob = with_and_without(args, tmp_path)
        assert rc != 0 and err and blob == b""
