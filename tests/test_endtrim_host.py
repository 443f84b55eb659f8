"""The host core of --trim_ends_q (csrc/endtrim.h) without a GPU: tests/endtrim_host.cpp runs it as a stand-alone program, built with
-O2 and again with the address and undefined-behaviour sanitizers (no preload, no Python, no GPU; every read sits in a heap block of
exactly its size).  Held, for equality, against tests/_endtrim_model.py.  The walk in pieces of 1, 7, 64 and the span, combined in order
by the associative rule, must give the serial walk's cuts: the decomposition the kernel relies on, tested — on random quality strings
and on strings with flat stretches (w = 0) and exact ties, where only the rule "the later piece wins only when strictly greater" gives
the serial answer."""
import os
import struct
import subprocess

import numpy as np
import pytest

import _endtrim_cases as cases
import _endtrim_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILDS = {"O2": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover"]}


@pytest.fixture(scope="module", params=sorted(BUILDS))
def program(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("endtrim_" + request.param) / "endtrim_host")
    subprocess.check_call(["g++", "-std=c++17"] + BUILDS[request.param] + ["-I" + os.path.join(ROOT, "filtlong_amd", "csrc"), "-o", exe,
                                                                          os.path.join(ROOT, "tests", "endtrim_host.cpp")])
    return exe


def span_of(exe):
    return int(subprocess.check_output([exe, "consts"]))


def walk(exe, tmp_path, reads, t):
    """per read five pairs (h, c): the serial walk, then pieces of 1, 7, 64 and the span"""
    src, dst = str(tmp_path / "in"), str(tmp_path / "out")
    with open(src, "wb") as f:
        f.write(struct.pack("<QQ", t, len(reads)))
        for r in reads:
            f.write(struct.pack("<Q", len(r)) + bytes(r))
    p = subprocess.run([exe, "walk", src, dst], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    blob = open(dst, "rb").read()
    assert len(blob) == 40 * len(reads)
    return np.frombuffer(blob, dtype="<u4").reshape(len(reads), 5, 2)


def compare(got, reads, t):
    for i, r in enumerate(reads):
        want = model.cuts(r, t)
        for k, how in enumerate(("serial walk", "pieces of 1", "pieces of 7", "pieces of 64", "pieces of the span")):
            assert tuple(int(x) for x in got[i, k]) == want, (how, i, len(r), got[i, k], want)


def test_the_model_agrees_with_itself():
    rng = np.random.default_rng(1)
    for r in cases.edge_reads(rng, 300) + cases.flat_reads(rng, 300):
        for t in (cases.T90, cases.T_PLUS, cases.T_MID, 0, 2**32 - 1):
            assert model.cuts(r, t) == model.cuts_walk(r, t)
    assert int(model.table()[43]) == cases.T_PLUS and int(model.table()[33]) == cases.E_BANG and int(model.table()[73]) == cases.E_I


@pytest.mark.parametrize("t", [cases.T90, cases.T_PLUS, 42949672, 3865470566, 0, 2**32 - 1])
def test_edges_and_random(program, tmp_path, t):
    span = span_of(program)
    assert span == 16384
    reads = cases.edge_reads(np.random.default_rng(5), span) + cases.any_bytes(np.random.default_rng(6))
    got = walk(program, tmp_path, reads, t)
    compare(got, reads, t)
    if t == cases.T90:
        assert sum(1 for g in got if g[0, 0] > 0) > 5 and sum(1 for g in got if g[0, 1] > 0) > 5


def test_flat_stretches_and_ties(program, tmp_path):
    span = span_of(program)
    reads = cases.flat_reads(np.random.default_rng(7), span)
    got = walk(program, tmp_path, reads, cases.T_PLUS)
    compare(got, reads, cases.T_PLUS)
    # (three '!' outweigh ten 'I', so the OTHER cut of these two takes the whole read: both cuts are over the whole read)
    assert tuple(got[0, 0]) == (0, 0) and tuple(got[2, 0]) == (3, 18) and tuple(got[3, 0]) == (18, 3)
    ties = cases.span_edge_ties(span)
    for t in (cases.T_MID, cases.T_PLUS):
        some = [r for r, tt in ties if tt == t]
        compare(walk(program, tmp_path, some, t), some, t)
    for idx, comp, value in cases.span_edge_tie_answers(span):
        r, t = ties[idx]
        assert model.cuts(r, t)[comp] == value, (idx, comp)


def test_five_spans_and_middle_junk(program, tmp_path):
    span = span_of(program)
    reads = [cases.five_spans(span, where, side) for side in (0, 1) for where in (0, 2, 4)] + [cases.middle_junk(True), cases.middle_junk(False)]
    got = walk(program, tmp_path, reads, cases.T90)
    compare(got, reads, cases.T90)
    for k, (side, where) in enumerate([(s, w) for s in (0, 1) for w in (0, 2, 4)]):
        at = int(got[k, 0, 0]) if side == 0 else len(reads[k]) - int(got[k, 0, 1])
        assert at // span == where  # the maximum lies in the span it was put in
    assert got[6, 0, 0] == 230 and tuple(got[7, 0]) == (0, 0)
