"""The host walk of --trim_adapters (csrc/adapters.h) without a GPU: tests/adapters_host.cpp runs it as a stand-alone program, built with
-O2 and again with the address and undefined-behaviour sanitizers (no preload, no Python, no GPU; every read sits in a heap block of
exactly its size).  Held, for equality, against tests/_adapters_model.py — the plain dynamic programme, not the bit-vector form."""
import os
import struct
import subprocess

import numpy as np
import pytest

import _adapters_cases as cases
import _adapters_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILDS = {"O2": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover"]}


@pytest.fixture(scope="module", params=sorted(BUILDS))
def program(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("adapters_" + request.param) / "adapters_host")
    subprocess.check_call(["g++", "-std=c++17"] + BUILDS[request.param] + ["-I" + os.path.join(ROOT, "filtlong_amd", "csrc"), "-o", exe,
                                                                          os.path.join(ROOT, "tests", "adapters_host.cpp")])
    return exe


def run(exe, tmp_path, seqs, errors, window, reads):
    """(build's answer, patterns [(m, k, head bases, tail bases)], per read (head key, tail key, children, first, last))"""
    src, dst = str(tmp_path / "in"), str(tmp_path / "out")
    with open(src, "wb") as f:
        f.write(struct.pack("<iiQ", errors, window, len(seqs)))
        for s in seqs:
            f.write(struct.pack("<Q", len(s)) + bytes(s))
        f.write(struct.pack("<Q", len(reads)))
        for r in reads:
            f.write(struct.pack("<Q", len(r)) + bytes(r))
    p = subprocess.run([exe, "run", src, dst], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    blob = open(dst, "rb").read()
    rc, = struct.unpack_from("<q", blob, 0)
    if rc != 0:
        assert len(blob) == 8
        return rc, [], []
    n, = struct.unpack_from("<Q", blob, 8)
    at, pats = 16, []
    for _ in range(n):
        m, k = struct.unpack_from("<II", blob, at)
        pats.append((m, k, blob[at + 8:at + 8 + m], blob[at + 8 + m:at + 8 + 2 * m]))
        at += 8 + 2 * m
    out = [struct.unpack_from("<IIiii", blob, at + 20 * i) for i in range(len(reads))]
    assert len(blob) == at + 20 * len(reads)
    return rc, pats, out


def want(seqs, errors, window, reads):
    pats = model.patterns(seqs)
    out = []
    for r in reads:
        kh, kt = model.end_key(r, 0, window, pats, errors), model.end_key(r, 1, window, pats, errors)
        ch, first, last = model.child_of(len(r), kh, kt)
        out.append((kh, kt, len(ch), first, last))
    return out


def test_byte_classes(program, tmp_path):
    out = str(tmp_path / "bytes")
    subprocess.check_call([program, "bytes", out])
    expect = bytearray(b"\x04" * 256)
    for i, c in enumerate(b"ACGT"):
        expect[c] = expect[c + 32] = i
    assert open(out, "rb").read() == bytes(expect)


def test_patterns_and_edits(program, tmp_path):
    rng = np.random.default_rng(5)
    seqs = [cases.random_adapter(rng, m) for m in (12, 13, 31, 32, 33, 63, 64)] + [b"acgtacgtacgtTTGA", cases.LIGATION]
    for errors in (0, 1, 20, 33, 40):
        rc, pats, _ = run(program, tmp_path, seqs, errors, 150, [])
        assert rc == 0 and len(pats) == 2 * len(seqs)
        for (m, k, head, tail), q in zip(pats, model.patterns(seqs)):
            assert (m, k, head, tail) == (len(q), len(q) * errors // 100, q, q[::-1])
    assert model.patterns([b"AACG" * 3])[1] == b"CGTT" * 3  # pattern 2 i + 1 is the reverse complement


def test_what_build_refuses(program, tmp_path):
    good = b"ACGTACGTACGTAA"
    for seqs, errors, window, answer in (([good, b"ACGTACGTACG"], 20, 150, 2), ([b"A" * 65], 20, 150, 1), ([good, good, b"ACGTACGTACGTNA"], 20, 150, 3),
                                         ([b"ACGTACGTACGTRA"], 20, 150, 1), ([good] * 129, 20, 150, -1), ([good], 41, 150, -1),
                                         ([good], -1, 150, -1), ([good], 20, 0, -1), ([good], 20, 1025, -1)):
        assert run(program, tmp_path, seqs, errors, window, [])[0] == answer
    assert run(program, tmp_path, [good] * 128, 40, 1024, [])[0] == 0 == run(program, tmp_path, [good], 0, 1, [])[0]


@pytest.mark.parametrize("window,errors", [(1, 20), (16, 0), (40, 20), (150, 40)])
def test_keys_and_children(program, tmp_path, window, errors):
    rng = np.random.default_rng(100 + window)
    seqs = [cases.LIGATION, cases.random_adapter(rng, 12), cases.random_adapter(rng, 33)]
    reads = cases.reads_for(rng, seqs, window)
    rc, _, got = run(program, tmp_path, seqs, errors, window, reads)
    assert rc == 0
    expect = want(seqs, errors, window, reads)
    assert got == expect
    if window >= 28:
        assert any(g[2] == 1 for g in got) and any(g[3] == -1 for g in got) and any(g[0] == 0 and g[1] == 0 for g in got)


def test_ties(program, tmp_path):
    """two patterns that end at the same j: the pattern index decides; a homopolymer, where every j ties: the largest wins"""
    x = b"GATTACAGATTACACCGTAG"
    seqs = [x, x[4:], b"A" * 12]
    reads = [x + b"CCCCCCCCCCCCCCCCCCCCCCCCCCCCCC", b"A" * 40 + b"CCGG" * 10, b"C" + b"A" * 200]
    rc, _, got = run(program, tmp_path, seqs, 0, 150, reads)
    assert rc == 0 and got == want(seqs, 0, 150, reads)
    assert got[0][0] == (20 << 8) | 2  # x[4:] is pattern 2 and ends where x (pattern 0) ends
    assert got[1][0] == (40 << 8) | 4  # poly-A: j = 12 .. 40 all have d = 0
    assert got[2][0] == (150 << 8) | 4 and got[2][1] >> 8 == 150 and got[2][2:] == (0, -1, -1)


def test_wide(program, tmp_path):
    """W = 1024 and 64-base patterns: every bit of the word, a text as long as a text gets"""
    rng = np.random.default_rng(9)
    seqs = [cases.random_adapter(rng, 64), cases.random_adapter(rng, 63)]
    reads = [cases.random_seq(rng, 960) + seqs[0] + cases.random_seq(rng, 3000), cases.random_seq(rng, 961) + seqs[0] + cases.random_seq(rng, 50),
             cases.random_seq(rng, 2000) + cases.substitute(rng, seqs[1], 6) + cases.random_seq(rng, 900)]
    rc, _, got = run(program, tmp_path, seqs, 20, 1024, reads)
    assert rc == 0 and got == want(seqs, 20, 1024, reads)
    assert got[0][0] == (1024 << 8) | 0 and got[2][1] != 0
