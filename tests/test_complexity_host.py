"""The host core of --max_low_complexity (csrc/complexity.h) without a GPU: tests/complexity_host.cpp runs it as a stand-alone program,
built with -O2 and again with the address and undefined-behaviour sanitizers (no preload, no Python, no GPU; every read sits in a heap
block of exactly its size).  Held, for equality, against tests/_complexity_model.py — the triplet histogram of every window from
scratch.  The piece-wise walks (pieces of 64 window starts, of a lane's run and of the span, a fresh state 63 bases in front of the end
of each piece's first window) must give the whole-read walk's count: the decomposition the kernel relies on, tested."""
import os
import struct
import subprocess

import numpy as np
import pytest

import _complexity_cases as cases
import _complexity_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILDS = {"O2": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover"]}


@pytest.fixture(scope="module", params=sorted(BUILDS))
def program(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("complexity_" + request.param) / "complexity_host")
    subprocess.check_call(["g++", "-std=c++17"] + BUILDS[request.param] + ["-I" + os.path.join(ROOT, "filtlong_amd", "csrc"), "-o", exe,
                                                                          os.path.join(ROOT, "tests", "complexity_host.cpp")])
    return exe


def consts(exe):
    window, warmup, run, span = map(int, subprocess.check_output([exe, "consts"]).split())
    return window, warmup, run, span


def walk(exe, tmp_path, reads, T, piece):
    """per read (S of the first window, windows, bad, bad by pieces of 64, by pieces of `piece`, by the kernel's spans and lane runs,
    bad(S, T) of the first window)"""
    src, dst = str(tmp_path / "in"), str(tmp_path / "out")
    with open(src, "wb") as f:
        f.write(struct.pack("<IIQ", T, piece, len(reads)))
        for r in reads:
            f.write(struct.pack("<Q", len(r)) + bytes(r))
    p = subprocess.run([exe, "walk", src, dst], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    blob = open(dst, "rb").read()
    assert len(blob) == 28 * len(reads)
    return [struct.unpack_from("<iIIIIII", blob, 28 * i) for i in range(len(reads))]


_WANT = {}  # the model's answers, shared by the two builds of the program


def compare(got, reads, T):
    for i, (r, g) in enumerate(zip(reads, got)):
        key = (r, T)
        if key not in _WANT:
            S, valid = model.window_scores(r)
            _WANT[key] = (int(np.count_nonzero(valid & model.is_bad(S, T))), (int(S[0]) if valid[0] else -1) if len(S) else -2)
        bad, s0 = _WANT[key]
        assert g[0] == s0, (i, len(r))
        assert g[1] == model.windows(len(r)), (i, len(r))
        assert g[2] == bad, ("whole read", i, len(r), g[2], bad)
        assert g[3] == bad, ("pieces of 64", i, len(r), g[3], bad)
        assert g[4] == bad, ("pieces", i, len(r), g[4], bad)
        assert g[5] == bad, ("spans and lane runs", i, len(r), g[5], bad)
        assert g[6] == (1 if s0 >= 0 and model.is_bad(s0, T) else 0), (i, len(r))


def test_constants(program):
    window, warmup, run, span = consts(program)
    assert (window, warmup) == (64, 63) and span == 64 * run and span % 64 == 0


@pytest.mark.parametrize("T", [10, 20, 37, 300])
def test_edges(program, tmp_path, T):
    _, _, run, span = consts(program)
    reads = cases.edge_reads(np.random.default_rng(5), span)
    for piece in (span, run, 16, 48):
        got = walk(program, tmp_path, reads, T, piece)
        compare(got, reads, T)
    by_read = dict(zip(reads, got))
    assert by_read[b"A" * 64][1:3] == (1, 1) and by_read[b"A" * 63][1:3] == (0, 0) and by_read[b"N" * 300][2] == 0
    assert sum(g[2] > 0 for g in got) > (len(reads) // 3 if T < 300 else 3)  # (at 300 only a homopolymer window is bad)


def test_mixed(program, tmp_path):
    _, _, run, span = consts(program)
    reads = cases.mixed_batch(np.random.default_rng(6), 60)
    compare(walk(program, tmp_path, reads, 20, run), reads, 20)


@pytest.mark.parametrize("T", [10, 20, 300])
def test_borderline(program, tmp_path, T):
    """S = floor(T * 61 / 10) is good and one more is bad (1831, one more than the edge of T = 300, is the score of no window)"""
    good, bad = model.borderline(np.random.default_rng(T), T)
    assert good is not None and (bad is not None or T == 300)
    reads = cases.borderline_reads(np.random.default_rng(T), T)
    got = walk(program, tmp_path, reads, T, 128)
    compare(got, reads, T)
    edge = T * 61 // 10
    assert got[0][0] == edge and got[0][2] == 0 and got[0][6] == 0
    if bad is not None:
        assert got[2][0] == edge + 1 and got[2][2] == 1 and got[2][6] == 1
