"""Unaligned BAM through the whole command line: for x.bam against x.fastq (the text tests/_bam.py expects), stdout, stderr (without
the FLX_CLI_BAM_TIMING line) and the exit status are identical — Phred mode, k-mer mode with --trim --split, --verbose, --report,
--gzip and --gpus 2 — at both values of FLX_CLI_GPU_BAM; the timing line names `device` at 1 and `host` at 0."""
import os
import re
import subprocess

import pytest

import _bam
import _bam_cases as bam_cases
import _bgzf
import _cases
import _e2e_checks

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "filtlong_amd", "bin", "filtlong")
TIMING = re.compile(rb"\[bam\] (\d+) record\(s\), (\d+) skipped, (device|host), [0-9.]+ ms\n")


def run(args, extra=None):
    env = dict(os.environ, LANG="C", LC_ALL="C")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    env.update(extra or {})
    p = subprocess.run([BIN] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
    return p.returncode, p.stdout, p.stderr


def records_of_fastq(blob):
    """(BAM's 4-bit codes have no letter case: the soft-masked bases of the k-mer reads become capitals in both inputs)"""
    lines = blob.split(b"\n")
    return [_bam.rec(lines[i][1:], lines[i + 1].decode().upper(), bytes(c - 33 for c in lines[i + 3])) for i in range(0, len(lines) - 3, 4)]


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    d = tmp_path_factory.mktemp("bam_inputs")
    f = {}

    def put(name, data):
        (d / name).write_bytes(data)
        f[name] = str(d / name)

    def pair(name, records):
        put(name + ".fastq", _bam.expected_fastq(records)[0])
        put(name + ".bam", _bam.bgzf(_bam.bam_bytes(records)))

    c1 = records_of_fastq(_cases.c1_fastq_bytes(n=300))
    # a few records the transcode treats differently: reversed, skipped, without qualities
    c1[3]["flag"] = 0x10
    c1[7]["flag"] = 0x100
    c1[11]["flag"] = 0x800
    c1.insert(20, _bam.rec(b"empty", "", b""))
    c1[30]["qual"] = None
    pair("c1", c1)
    inp = _e2e_checks.Inputs()
    pair("kmer", records_of_fastq(_cases.long_fastq_bytes(inp.kreads)))
    put("ref.fasta", _cases.fasta_bytes(inp.contigs))
    for c in bam_cases.corpus():
        if c.name in ("lengths", "long"):
            pair(c.name, list(c.records))
    return f


def both_switches(args, inputs, name, extra=None, n_skipped=None):
    """the run on NAME.fastq, and the runs on NAME.bam at both switch values: identical but for the timing line"""
    def with_input(suffix):
        return [a.replace("{in}", inputs[name + suffix]) for a in args]
    plain = run(with_input(".fastq"), extra)
    for switch, path in (("0", b"host"), ("1", b"device")):
        rc, out, err = run(with_input(".bam"), dict(extra or {}, FLX_CLI_GPU_BAM=switch, FLX_CLI_BAM_TIMING="1"))
        lines = TIMING.findall(err)
        assert len(lines) == 1 and lines[0][2] == path, (switch, err[-600:])
        if n_skipped is not None:
            assert int(lines[0][1]) == n_skipped
        err = TIMING.sub(b"", err).replace(b".bam", b".fastq")
        assert (rc, out, err) == plain, (switch, rc, plain[0], err[-400:], plain[2][-400:])
    return plain


def test_phred(inputs):
    for args in (["--keep_percent", "80"], ["--target_bases", "300000"], ["--min_length", "4000", "--min_mean_q", "80"]):
        rc, out, err = both_switches(args + ["{in}"], inputs, "c1", n_skipped=3)
        assert rc == 0 and out
    rc, out, err = both_switches(["--keep_percent", "90", "{in}"], inputs, "lengths")
    assert rc == 0 and out
    rc, out, err = both_switches(["--min_length", "1", "{in}"], inputs, "long")
    assert rc == 0 and out.count(b"\n") == 12  # (all three records pass, the 300 000-base one among them)


def test_kmer_trim_split(inputs):
    rc, out, err = both_switches(["-a", inputs["ref.fasta"], "--trim", "--split", "100", "--keep_percent", "80", "{in}"], inputs, "kmer")
    assert rc == 0 and out


def test_verbose(inputs):
    rc, out, err = both_switches(["--verbose", "--target_bases", "200000", "{in}"], inputs, "c1")
    assert rc == 0 and out and len(err) > 10000


def test_report(inputs, tmp_path):
    reports = {}
    for suffix, switch in ((".fastq", "0"), (".bam", "0"), (".bam", "1")):
        rep = tmp_path / ("report%s%s.json" % (suffix, switch))
        res = run(["--report", str(rep), "--keep_percent", "70", inputs["c1" + suffix]], {"FLX_CLI_GPU_BAM": switch})
        assert res[0] == 0
        reports[(suffix, switch)] = (res[1], rep.read_bytes().replace(b".bam", b".fastq"))
    assert reports[(".bam", "0")] == reports[(".fastq", "0")] == reports[(".bam", "1")] and reports[(".bam", "1")][1]


def test_gzip(inputs):
    outs = []
    for suffix, switch in ((".fastq", "0"), (".bam", "0"), (".bam", "1")):
        rc, out, err = run(["--gzip", "--keep_percent", "70", inputs["c1" + suffix]], {"FLX_CLI_GPU_BAM": switch})
        assert rc == 0
        outs.append(_bgzf.validate(out)[0])
    assert outs[0] == outs[1] == outs[2] and outs[0]


def test_two_ranks(inputs):
    shim_dir = os.path.join(ROOT, "tests", "shim")
    subprocess.check_call(["make", "-s", "-C", shim_dir])
    extra = {"FLX_RCCL_LIB": os.path.join(shim_dir, "libloopback_rccl.so"), "FLX_DEVICE": "0"}
    rc, out, err = both_switches(["--gpus", "2", "--target_bases", "300000", "{in}"], inputs, "c1", extra)
    assert rc == 0 and out
    assert (rc, out) == run(["--target_bases", "300000", inputs["c1.bam"]])[:2]


def test_damaged_is_refused_by_both_paths(inputs, tmp_path):
    good = _bam.bam_bytes(bam_cases.three_records() * 5)
    for how, blob in (("truncated", good[:-9]), ("malformed", dict(bam_cases.damaged())["l_read_name_0"])):
        bam, rep = tmp_path / (how + ".bam"), tmp_path / (how + ".json")
        bam.write_bytes(_bam.bgzf(blob))
        for switch in "01":
            rc, out, err = run(["--report", str(rep), "--min_length", "1", str(bam)], {"FLX_CLI_GPU_BAM": switch})
            assert rc == 1 and out == b"" and rep.read_bytes() == b""
            assert b"Error: could not read BAM input " + str(bam).encode() + b": " in err
