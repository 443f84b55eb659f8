"""The BAM record core of csrc/bam_record.h without a GPU: tests/bam_host.cpp walks it on the host, built with -O2 and again with the
address and undefined-behaviour sanitizers (a stand-alone program: no preload, no Python, no GPU).  The whole corpus of
tests/_bam_cases.py gives the text, the offsets and the skip count tests/_bam.py expects, each input in a heap block of exactly its
size; damaged inputs give the end state and the records of tests/_bam.py's model of the walk, and never a read outside the block —
the sanitizer build is the proof."""
import os
import struct
import subprocess

import pytest

import _bam
import _bam_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILDS = {"O2": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover"]}


def build_host_program(flags, exe):
    subprocess.check_call(["g++", "-std=c++17"] + flags + ["-I" + os.path.join(ROOT, "filtlong_amd", "csrc"), "-o", exe,
                                                           os.path.join(ROOT, "tests", "bam_host.cpp")])
    return exe


def run_host_program(exe, tmp_path, files):
    """[(end state, records, skipped, text, offsets)] of the inflated files"""
    src, dst = str(tmp_path / "corpus"), str(tmp_path / "results")
    with open(src, "wb") as f:
        f.write(struct.pack("<I", len(files)))
        for b in files:
            f.write(struct.pack("<I", len(b)) + b)
    p = subprocess.run([exe, src, dst], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    blob, at, out = open(dst, "rb").read(), 0, []
    for _ in files:
        end, n, skipped, length = struct.unpack_from("<IQQQ", blob, at)
        at += 28
        text = blob[at:at + length]
        at += length
        off = list(struct.unpack_from("<%dQ" % (n + 1), blob, at))
        at += 8 * (n + 1)
        out.append((end, n, skipped, text, off))
    assert at == len(blob)
    return out


@pytest.fixture(scope="module", params=sorted(BUILDS))
def program(request, tmp_path_factory):
    return build_host_program(BUILDS[request.param], str(tmp_path_factory.mktemp("bam_" + request.param) / "bam_host"))


@pytest.fixture(scope="module")
def corpus():
    return cases.corpus()


def test_corpus(program, corpus, tmp_path):
    res = run_host_program(program, tmp_path, [cases.case_bam(c) for c in corpus])
    for c, (end, n, skipped, text, off) in zip(corpus, res):
        want_text, want_off, want_skipped = _bam.expected_fastq(c.records)
        assert (end, n, skipped) == (_bam.END, len(c.records), want_skipped), c.name
        assert off == want_off, c.name
        assert text == want_text, c.name
    assert len(corpus) >= 20 and any(len(r["seq"]) == cases.LONG for c in corpus for r in c.records)


def test_damaged(program, tmp_path):
    files = cases.damaged()
    res = run_host_program(program, tmp_path, [b for _, b in files])
    ends = set()
    for (name, b), (end, n, skipped, text, off) in zip(files, res):
        want_records, want_end = _bam.walk_model(b)
        assert (end, n) == (want_end, len(want_records)), name
        assert (text, off, skipped) == _bam.expected_fastq(want_records), name
        ends.add(end)
    assert ends == {_bam.END, _bam.TRUNCATED, _bam.MALFORMED, _bam.HEADER}
    by_name = {name: r[0] for (name, _), r in zip(files, res)}
    # the rules one by one: each breaks the walk at record 1
    for name in ("block_size_31", "l_read_name_0", "name_without_nul", "l_seq_-1", "l_seq_-2147483648", "l_seq_2147483647", "l_seq_65536",
                 "n_cigar_op_65535", "l_seq_and_n_cigar_large", "block_size_short_by_1"):
        assert by_name[name] == _bam.MALFORMED and by_name[name + "_at_end"] == _bam.MALFORMED, name
    assert by_name["block_size_huge"] == _bam.TRUNCATED
    assert sum(1 for name, e in by_name.items() if name.startswith("cut_") and e == _bam.TRUNCATED) >= len([1 for n, _ in files if n.startswith("cut_")]) - 4
    assert sum(1 for name, e in by_name.items() if name.startswith("fuzz_") and e != _bam.END) >= 50
    assert sum(1 for name, _ in files if name.startswith("fuzz_")) == 200
