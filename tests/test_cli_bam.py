"""Unaligned BAM as the input of the command line, without a GPU: with FLX_CLI_GPU_BAM=0 the FLX_CLI_PARSE_ONLY digests (sequential
and concurrent parser) of x.bam are those of x.fastq, the text tests/_bam.py expects — for the corpus in every BGZF layout and for
every reference fixture.  A truncated or malformed file gives the error line and status 1."""
import glob
import os
import subprocess

import pytest

import _bam
import _bam_cases as cases
import _cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "filtlong_amd", "bin", "filtlong")


def digest(path, mode, extra=None):
    env = dict(os.environ, LANG="C", LC_ALL="C", FLX_CLI_PARSE_ONLY=mode, FLX_CLI_GPU_BAM="0", FLX_CLI_PARALLEL_PARSE_MIN="1")
    env.update(extra or {})
    p = subprocess.run([BIN, "--min_length", "1", path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
    return p.returncode, p.stdout, p.stderr


@pytest.fixture(scope="module")
def binary():
    if not os.path.exists(BIN):
        import __graft_entry__
        __graft_entry__.build()
    return BIN


def same_digests(tmp_path, name, bam_file, text):
    fq, bam = tmp_path / (name + ".fastq"), tmp_path / (name + ".bam")
    fq.write_bytes(text)
    bam.write_bytes(bam_file)
    for mode in ("seq", "par"):
        want = digest(str(fq), mode)
        assert want[0] == 0, want[2]
        assert digest(str(bam), mode) == want, (name, mode)
    return digest(str(fq), "seq")[1]


def test_corpus_in_every_layout(binary, tmp_path):
    layouts = set()
    for c in cases.corpus():
        text = _bam.expected_fastq(c.records)[0]
        for layout, blob in cases.bgzf_layouts(c).items():
            out = same_digests(tmp_path, c.name + "_" + layout, blob, text)
            layouts.add(layout)
        kept = sum(_bam.has_text(r) for r in c.records)
        assert out.startswith(b"records %d status -1 " % kept), (c.name, out)
    assert layouts == {"default", "no_eof", "straddle", "member_per_record"}


def test_reference_fixtures(binary, tmp_path):
    fixtures = sorted(glob.glob(os.path.join(_cases.FIXTURES, "*.fastq")))
    assert len(fixtures) >= 4
    for path in fixtures:
        records = _bam.read_fastq(path)
        assert len(records) >= 3
        same_digests(tmp_path, os.path.basename(path)[:-6], _bam.bgzf(_bam.bam_bytes(records)), _bam.expected_fastq(records)[0])
    # ... and the text of a well-formed fixture is the fixture
    good = os.path.join(_cases.FIXTURES, "test_sort.fastq")
    assert _bam.expected_fastq(_bam.read_fastq(good))[0] == open(good, "rb").read()


def test_timing_line_names_the_host(binary, tmp_path):
    c = cases.corpus()[0]
    bam = tmp_path / "x.bam"
    bam.write_bytes(_bam.bgzf(cases.case_bam(c)))
    rc, out, err = digest(str(bam), "seq", {"FLX_CLI_BAM_TIMING": "1"})
    assert rc == 0 and b"[bam] %d record(s), 0 skipped, host, " % len(c.records) in err, err
    assert b"[bam]" not in digest(str(bam), "seq", {"FLX_CLI_BAM_TIMING": "0"})[2]
    for bad in ("2", "yes", ""):
        rc, out, err = digest(str(bam), "seq", {"FLX_CLI_GPU_BAM": bad})
        assert rc == 1 and not out and b"FLX_CLI_GPU_BAM must be 0 or 1" in err


def test_only_a_bgzf_file_with_the_magic_is_bam(binary, tmp_path):
    """a gzip file that is no BAM, and a plain file that starts with the magic, are what they were"""
    text = _bam.expected_fastq(cases.corpus()[0].records)[0]
    gz, fq = tmp_path / "t.fastq.gz", tmp_path / "t.fastq"
    gz.write_bytes(_bam.bgzf(text))
    fq.write_bytes(text)
    assert digest(str(gz), "seq") == digest(str(fq), "seq")
    plain = tmp_path / "plain.bam"
    plain.write_bytes(cases.case_bam(cases.corpus()[0]))  # not compressed: no BAM input
    rc, out, err = digest(str(plain), "seq")
    assert rc == 0 and b"could not read BAM" not in err


DAMAGED = ["truncated_in_record", "truncated_in_header", "block_size_31", "l_read_name_0", "name_without_nul", "l_seq_-1", "no_magic_behind_detection",
           "l_text_negative", "member_bit_flip", "member_cut"]


@pytest.mark.parametrize("how", DAMAGED)
def test_damaged(binary, tmp_path, how):
    recs = cases.three_records()
    good = _bam.bam_bytes(recs)
    by_name = dict(cases.damaged())
    if how == "truncated_in_record":
        blob = _bam.bgzf(good[:-7])
    elif how == "truncated_in_header":
        blob = _bam.bgzf(good[:9], eof=False)
    elif how == "no_magic_behind_detection":  # the first member says BAM, the header's lengths do not hold
        blob = _bam.bgzf(b"BAM\1" + b"\xff\xff\xff\x7f" + good[8:])
    elif how == "member_bit_flip":
        b = bytearray(_bam.bgzf(good + good, member=150))
        b[len(_bam.bgzf_member((good + good)[:150])) + 40] ^= 0x10
        blob = bytes(b)
    elif how == "member_cut":
        blob = _bam.bgzf(good + good, member=150, eof=False)[:-30]
    else:
        blob = _bam.bgzf(by_name[how])
    bam = tmp_path / (how + ".bam")
    bam.write_bytes(blob)
    for mode in ("seq", "par"):
        rc, out, err = digest(str(bam), mode)
        assert rc == 1 and out == b"", (rc, out, err)
        assert err.startswith(b"Error: could not read BAM input " + str(bam).encode() + b": ") and err.count(b"\n") == 1, err
