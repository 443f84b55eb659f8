"""The BAM writer's record core (csrc/bam_encode.h) without a GPU: tests/bam_encode_host.cpp walks it on the host, built with -O2
and again with the address and undefined-behaviour sanitizers (a stand-alone program: no preload, no Python, no GPU).  The corpus of
tests/_bam_encode_cases.py gives, byte for byte, the records of the independent writer in tests/_bam.py; each damaged shape names
its record as the first bad one; and bam_record.h's host walk over the encoded records gives the text back, the name cut at its
first blank and the bases upper-cased through the table.  The header and the bound are checked against the library (no device is
needed for either; it is built first when it is missing)."""
import os
import struct
import subprocess

import pytest

import _bam
import _bam_encode_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILDS = {"O2": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover"]}


def build_host_program(flags, exe):
    subprocess.check_call(["g++", "-std=c++17"] + flags + ["-I" + os.path.join(ROOT, "filtlong_amd", "csrc"), "-o", exe,
                                                           os.path.join(ROOT, "tests", "bam_encode_host.cpp")])
    return exe


def run_host_program(exe, tmp_path, inputs):
    """inputs: [(text, rec_off)] -> [(first_bad, records, offsets, text back)]"""
    src, dst = str(tmp_path / "corpus"), str(tmp_path / "results")
    with open(src, "wb") as f:
        f.write(struct.pack("<I", len(inputs)))
        for text, off in inputs:
            f.write(struct.pack("<I%dQI" % len(off), len(off) - 1, *off, len(text)) + text)
    p = subprocess.run([exe, src, dst], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    blob, at, out = open(dst, "rb").read(), 0, []
    for text, off in inputs:
        first_bad, length = struct.unpack_from("<QQ", blob, at)
        at += 16
        rec = blob[at:at + length]
        at += length
        out_off = list(struct.unpack_from("<%dQ" % len(off), blob, at))
        at += 8 * len(off)
        back_len, = struct.unpack_from("<Q", blob, at)
        at += 8
        back = blob[at:at + back_len]
        at += back_len
        out.append((first_bad, rec, out_off, back))
    assert at == len(blob)
    return out


@pytest.fixture(scope="module", params=sorted(BUILDS))
def program(request, tmp_path_factory):
    return build_host_program(BUILDS[request.param], str(tmp_path_factory.mktemp("bamenc_" + request.param) / "bam_encode_host"))


def test_corpus(program, tmp_path):
    corpus = cases.corpus()
    res = run_host_program(program, tmp_path, [cases.text_of(c.entries) for c in corpus])
    for c, (first_bad, rec, off, back) in zip(corpus, res):
        want, want_off = cases.expected_bam(c.entries)
        assert first_bad == len(c.entries), c.name
        assert off == want_off, c.name
        assert rec == want, c.name
        # the round trip: names without their comments, bases upper-cased through the table, '"' for a FASTA record's qualities
        assert back == _bam.expected_fastq(cases.expected_records(c.entries))[0], c.name
        # what the specification's walk makes of a file of these records
        records, end = _bam.walk_model(_bam.header_bytes() + rec)
        assert end == _bam.END and len(records) == len(c.entries), c.name
    lengths = {len(s) for c in corpus for _, _, s, _ in c.entries}
    assert lengths >= set(cases.LENGTHS) | {cases.LONG}
    by_name = {c.name: (c, r) for c, r in zip(corpus, res)}
    mixed, rec = by_name["mixed"][0], by_name["mixed"][1][1]
    assert mixed.entries[-1][0] == b">" and len(mixed.entries[-1][2]) % 2 == 1 and rec[-1] == 0xff  # a FASTA record: 0xFF qualities
    only, rec = by_name["last_odd_fastq"][0], by_name["last_odd_fastq"][1][1]
    l = len(only.entries[0][2])
    assert l % 2 == 1 and rec[len(rec) - l - 1] & 15 == 0  # an odd L as the last record: the low pad nibble is zero


def test_damaged(program, tmp_path):
    files = cases.damaged()
    res = run_host_program(program, tmp_path, [(t, off) for _, t, off, _ in files])
    for (name, t, off, want_bad), (first_bad, rec, out_off, back) in zip(files, res):
        assert first_bad == want_bad, name
    names = {n for n, _, _, _ in files}
    assert {"missing_plus", "odd_remainder", "newline_not_where_L_puts_it", "empty_name", "name_255", "qual_32_at_0", "qual_127_at_16"} <= names


def test_offsets_that_do_not_follow_the_records(program, tmp_path):
    text, off = cases.text_of(cases.corpus()[0].entries[:6])
    shifted = list(off)
    shifted[3] += 1
    past = list(off)
    past[-1] += 40
    back = list(off)
    back[2] = off[1] - 1
    res = run_host_program(program, tmp_path, [(text, shifted), (text, past), (text, back)])
    assert [r[0] for r in res] == [2, 5, 1]


def test_header_and_bound():
    if not os.path.exists(os.path.join(ROOT, "filtlong_amd", "lib", "libfiltlong_hip.so")):
        import __graft_entry__
        __graft_entry__.build()
    from filtlong_amd import api
    assert api.bam_header() == _bam.header_bytes(text=b"@HD\tVN:1.6\tSO:unknown\n")
    # the bound holds with equality nowhere below the records' sizes: L = 0 and 1-byte names are where a record grows the most
    for entries in ([(b">", b"x", b"", b"")], [(b"@", b"x", b"", b"")], [(b">", b"x", b"A", b"")], [(b"@", b"x", b"A", b"!")],
                    [(b">", b"x", b"", b"")] * 1000, [(b">", b"x", b"ACG", b"")] * 7, [c for case in cases.corpus() for c in case.entries]):
        text, off = cases.text_of(entries)
        assert len(cases.expected_bam(entries)[0]) <= api.bam_from_fastq_bound(len(text), len(entries)), entries[0]
    assert api.bam_from_fastq_bound(0, 0) == 0
