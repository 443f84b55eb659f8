"""The host walk of --split_adapters (csrc/adapters.h) without a GPU: tests/adapters_split_host.cpp runs it as a stand-alone program,
built with -O2 and again with the address and undefined-behaviour sanitizers (no preload, no Python, no GPU; every read and every
array of marks sits in a heap block of exactly its size).  Held, for equality, against tests/_adapters_split_model.py — the plain
dynamic programme over the whole read.  The piece-wise walk (pieces of 64 and of 1024 bases, a fresh column kWarmup bases in front of
each) must give the marks of the whole-read walk: the independence argument of DESIGN 4.12, tested."""
import os
import struct
import subprocess

import numpy as np
import pytest

import _adapters_model as model
import _adapters_split_cases as cases
import _adapters_split_model as split

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILDS = {"O2": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover"]}


@pytest.fixture(scope="module", params=sorted(BUILDS))
def program(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("adapters_split_" + request.param) / "adapters_split_host")
    subprocess.check_call(["g++", "-std=c++17"] + BUILDS[request.param] + ["-I" + os.path.join(ROOT, "filtlong_amd", "csrc"), "-o", exe,
                                                                          os.path.join(ROOT, "tests", "adapters_split_host.cpp")])
    return exe


def run(exe, tmp_path, seqs, errors, window, split_errors, reads):
    """per read (head key, tail key, first, last, children, marks, marks by pieces of 64, marks by pieces of 1024)"""
    src, dst = str(tmp_path / "in"), str(tmp_path / "out")
    with open(src, "wb") as f:
        f.write(struct.pack("<iiiiQ", errors, window, split_errors, 0, len(seqs)))
        for s in seqs:
            f.write(struct.pack("<Q", len(s)) + bytes(s))
        f.write(struct.pack("<Q", len(reads)))
        for r in reads:
            f.write(struct.pack("<Q", len(r)) + bytes(r))
    p = subprocess.run([exe, src, dst], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    blob = open(dst, "rb").read()
    assert struct.unpack_from("<q", blob, 0)[0] == 0
    at, out = 8, []
    for r in reads:
        kh, kt, n, first, last = struct.unpack_from("<IIiii", blob, at)
        at += 20
        ch = [tuple(struct.unpack_from("<ii", blob, at + 8 * k)) for k in range(n)]
        at += 8 * n
        m = [np.frombuffer(blob, dtype=np.uint8, count=len(r), offset=at + k * len(r)).astype(bool) for k in range(3)]
        at += 3 * len(r)
        out.append((kh, kt, first, last, ch, m[0], m[1], m[2]))
    assert at == len(blob)
    return out


_WANT = {}  # the model's answers, shared by the two builds of the program


def compare(got, seqs, errors, window, split_errors, reads):
    pats = model.patterns(seqs)
    key = (tuple(pats), errors, window, split_errors, tuple(reads))
    if key not in _WANT:
        _WANT[key] = [split.split_of(r, window, pats, errors, split_errors) for r in reads]
    for i, (r, g) in enumerate(zip(reads, got)):
        kh, kt, marks, ch, first, last = _WANT[key][i]
        assert (g[0], g[1]) == (kh, kt), i
        assert (g[5] == marks).all(), (i, len(r), np.nonzero(g[5] != marks)[0][:8].tolist())
        assert (g[6] == marks).all(), ("pieces of 64", i, len(r), np.nonzero(g[6] != marks)[0][:8].tolist())
        assert (g[7] == marks).all(), ("pieces of 1024", i, len(r), np.nonzero(g[7] != marks)[0][:8].tolist())
        assert (g[2], g[3], g[4]) == (first, last, ch), (i, len(r))


@pytest.mark.parametrize("split_errors", [0, 10, 40])
def test_placements(program, tmp_path, split_errors):
    """adapters on every edge of a piece and of its warm-up, patterns of 12, 33 and 64 bases"""
    rng = np.random.default_rng(300 + split_errors)
    for seqs in ([cases.LIGATION, cases.random_adapter(rng, 12)], [cases.random_adapter(rng, 64), cases.random_adapter(rng, 33)]):
        reads = cases.placements(rng, seqs, split_errors)
        got = run(program, tmp_path, seqs, 20, 60, split_errors, reads)
        compare(got, seqs, 20, 60, split_errors, reads)
        assert sum(len(g[4]) >= 2 for g in got) > len(reads) // 2
    if split_errors == 0:
        assert any(e - s == 1 for g in got for s, e in g[4])  # two adapters one base apart leave a child of one base


def test_small_pieces(program, tmp_path):
    """the same edges for pieces of 64 bases: the program walks every read in pieces of 64 as well"""
    rng = np.random.default_rng(64)
    seqs = [cases.random_adapter(rng, 31), cases.random_adapter(rng, 32), cases.random_adapter(rng, 64)]
    for split_errors in (10, 40):
        reads = cases.placements(rng, seqs, split_errors, S=64) + cases.placements(rng, seqs[2:], split_errors, S=64)
        compare(run(program, tmp_path, seqs, 20, 40, split_errors, reads), seqs, 20, 40, split_errors, reads)


def test_ends_rule(program, tmp_path):
    rng = np.random.default_rng(7)
    seqs = [cases.LIGATION, cases.random_adapter(rng, 16)]
    reads = cases.end_rule_reads(rng, seqs)
    got = run(program, tmp_path, seqs, 20, 60, 10, reads)
    compare(got, seqs, 20, 60, 10, reads)
    assert (got[7][2], got[7][3], got[7][4]) == (-1, -1, [])               # all adapter
    assert got[6][0] == 0 and got[6][1] == 0 and len(got[6][4]) == 2       # a middle hit without an end hit: two children
    assert got[4][0] != 0 and len(got[4][4]) == 1                          # an end hit: one child, the occurrence is marked too
    # without any adapter a read goes on as itself
    plain = [cases.random_seq(rng, 900), b"", b"N" * 30]
    for g, r in zip(run(program, tmp_path, seqs, 20, 60, 10, plain), plain):
        assert (g[2], g[3], g[4]) == (0, len(r), []) and not g[5].any()


def test_bytes(program, tmp_path):
    rng = np.random.default_rng(11)
    seqs = [b"AAAAAAAAAAAAAAAC", cases.LIGATION.lower(), b"A" * 12]
    reads = cases.byte_reads(rng, seqs)
    got = run(program, tmp_path, seqs, 20, 150, 10, reads)
    compare(got, seqs, 20, 150, 10, reads)
    assert got[11][5].all() and (got[11][2], got[11][3]) == (-1, -1)  # the homopolymer is one run of marks
