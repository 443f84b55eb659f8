"""The record core of --split_window_q (csrc/qsplit.h) without a GPU: tests/qsplit_host.cpp walks it on the host, built with -O2
and again with the address and undefined-behaviour sanitizers (a stand-alone program: no preload, no Python, no GPU; every quality
string sits in a heap block of exactly its size).  It is held, for equality, against tests/_qsplit_model.py: the table from 60-digit
decimals, the children as the runs of bases that no bad window covers.  Window sizes go to 5000: the sizes at which the GPU tests
hold the detection kernel against the same model (tests/test_qsplit_gpu_deep.py)."""
import os
import struct
import subprocess

import numpy as np
import pytest

import _qsplit_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILDS = {"O2": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover"]}


@pytest.fixture(scope="module", params=sorted(BUILDS))
def program(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("qsplit_" + request.param) / "qsplit_host")
    subprocess.check_call(["g++", "-std=c++17"] + BUILDS[request.param] + ["-I" + os.path.join(ROOT, "filtlong_amd", "csrc"), "-o", exe,
                                                                          os.path.join(ROOT, "tests", "qsplit_host.cpp")])
    return exe


def walk(exe, tmp_path, cases):
    """cases: [(w, t, qual)] -> [(ranges, first, last, any_bad)]"""
    src, dst = str(tmp_path / "cases"), str(tmp_path / "results")
    with open(src, "wb") as f:
        f.write(model.pack_cases(cases))
    p = subprocess.run([exe, "walk", src, dst], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    blob, at, out = open(dst, "rb").read(), 0, []
    for _ in cases:
        n, first, last, any_bad = struct.unpack_from("<QiiI", blob, at)
        at += 20
        flat = struct.unpack_from("<%di" % (2 * n), blob, at)
        at += 8 * n
        out.append(([(flat[2 * k], flat[2 * k + 1]) for k in range(n)], first, last, bool(any_bad)))
    assert at == len(blob)
    return out


def check(exe, tmp_path, cases):
    got = walk(exe, tmp_path, cases)
    for (w, t, s), g in zip(cases, got):
        assert g == model.children(s, w, t), (w, t, len(s))
    return got


def test_table_and_threshold(program, tmp_path):
    out = str(tmp_path / "table")
    subprocess.check_call([program, "table", out])
    table = list(struct.unpack("<256I", open(out, "rb").read()))
    assert table == model.error_table()
    assert table[ord('"')] == 3411613790 and table[ord("+")] == 429496730 and table[ord("~")] == 2
    assert table[ord("!")] == model.U32_MAX and table[0] == model.U32_MAX and table[255] == model.U32_MAX
    for q in (0.5, 1, 50, 85, 90, 99, 99.999):
        assert subprocess.check_output([program, "threshold", repr(float(q))]).decode().strip() == str(model.threshold(q))
    for q in (0, 100, 250):
        assert subprocess.check_output([program, "threshold", repr(float(q))]).decode().strip() == "invalid"


def test_lengths_around_the_window(program, tmp_path):
    rng = np.random.default_rng(11)
    cases = []
    for w in (1, 2, 7, 250, 1026, 2048, 5000):  # (the last three: windows deeper than one step of the detection kernel)
        for length in sorted({0, 1, max(w - 1, 0), w, w + 1, 2 * w - 1, 2 * w} | ({2 * w + 1, 3 * w + 7} if w > 1000 else set())):
            for q in (50, 85, 99):
                t = model.threshold(q)
                cases.append((w, t, model.junk_read(rng, length, [])))                      # nothing bad
                cases.append((w, t, model.junk_read(rng, length, [(0, length)])))           # everything bad
                cases.append((w, t, model.junk_read(rng, length, [(0, max(1, w // 2 + 1))])))  # a bad window first
                cases.append((w, t, model.junk_read(rng, length, [(length - w // 2 - 1, length)])))  # ... and last
                cases.append((w, t, rng.integers(33, 60, size=length).astype(np.uint8).tobytes()))
    got = check(program, tmp_path, cases)
    # (two children need 2 W + 1 bases: the other tests have them.)  Reads cut to one child, wholly bad reads, untouched reads:
    assert any(a and len(r) == 1 for r, _, _, a in got) and any(a and not r for r, _, _, a in got) and any(not a for _, _, _, a in got)
    assert any(r and r[0][0] > 0 for r, _, _, _ in got), "a bad window first"
    assert any(r and r[-1][1] < len(s) for (_, _, s), (r, _, _, _) in zip(cases, got)), "a bad window last"


def test_bad_ends_w_and_w_plus_1_apart(program, tmp_path):
    # W = 7, Q = 99: one '!' among '~' makes the seven windows that hold it bad, bad ends p .. p + 6
    w, t = 7, model.threshold(99)

    def read(length, bangs):
        s = bytearray(b"~" * length)
        for p in bangs:
            s[p] = ord("!")
        return bytes(s)

    got = check(program, tmp_path, [(w, t, read(60, [20, 20 + 13])), (w, t, read(60, [20, 20 + 14])), (w, t, read(60, [20]))])
    assert got[0][0] == [(0, 14), (40, 60)]            # bad ends 26 and 33 are W apart: no base between their windows, merged
    assert got[1][0] == [(0, 14), (27, 28), (41, 60)]  # W + 1 apart: a child of one base
    assert got[2][0] == [(0, 14), (27, 60)]


def test_whole_read_bad_and_every_byte(program, tmp_path):
    rng = np.random.default_rng(5)
    cases = []
    for w in (1, 2, 7, 250):
        for q in (50, 99):
            t = model.threshold(q)
            cases.append((w, t, b"!" * 600))
            cases.append((w, t, model.junk_read(rng, 600, [(0, 600)])))
            for _ in range(3):
                cases.append((w, t, rng.permutation(np.arange(256, dtype=np.uint8).repeat(3)).tobytes()))
            cases.append((w, t, bytes(range(256))))
    got = check(program, tmp_path, cases)
    for (w, t, s), (r, first, last, any_bad) in zip(cases, got):
        if s == b"!" * 600:
            assert (r, first, last, any_bad) == ([], -1, -1, True)


def test_the_issue_example(program, tmp_path):
    """W = 250, Q = 85: 3000 bases of Phred 12-34 with Phred 1-5 in [1000, 1400) split into two children, at about [0, 817) and
    [1584, 3000) (the boundaries depend on the draw: their order of magnitude is asserted)."""
    rng = np.random.default_rng(2024)
    s = model.junk_read(rng, 3000, [(1000, 1400)])
    (r, first, last, any_bad), = check(program, tmp_path, [(250, model.threshold(85), s)])
    assert len(r) == 2 and any_bad and first == 0 and last == 3000
    assert r[0][0] == 0 and 750 < r[0][1] <= 1000 and 1400 <= r[1][0] < 1650 and r[1][1] == 3000


def test_random_reads(program, tmp_path):
    rng = np.random.default_rng(77)
    cases = []
    for w in (1, 2, 7, 31, 250):
        for q in (50, 85, 90, 99):
            t = model.threshold(q)
            for _ in range(12):
                length = int(rng.integers(0, 3000))
                k = int(rng.integers(0, 4))
                st = [(a, a + int(rng.integers(1, 600))) for a in rng.integers(0, max(length, 1), size=k)]
                cases.append((w, t, model.junk_read(rng, length, st)))
    got = check(program, tmp_path, cases)
    assert sum(len(r) >= 2 for r, _, _, _ in got) > 20
    # windows deeper than one step of the detection kernel, reads up to 3 W + 7 bases, stretches up to W
    deep = []
    for w in (1026, 2048, 5000):
        for q in (50, 85, 90, 99):
            t = model.threshold(q)
            for i in range(12):
                length = int(rng.integers(0, 3 * w + 8))
                k = int(rng.integers(0, 4))
                st = [(a, a + int(rng.integers(1, w + 1))) for a in rng.integers(0, max(length, 1), size=k)]
                if i % 2:  # two children need 2 W + 1 bases and a stretch away from both ends
                    length = int(rng.integers(2 * w + 1, 3 * w + 8))
                    a = int(rng.integers(length // 2 - w // 4, length // 2))
                    st = [(a, a + int(rng.integers(w // 4, w // 2)))]
                deep.append((w, t, model.junk_read(rng, length, st)))
    got = check(program, tmp_path, deep)
    assert sum(len(r) >= 2 for r, _, _, _ in got) > 5
