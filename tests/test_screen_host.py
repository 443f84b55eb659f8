"""The host core of --exclude (csrc/screen.h) without a GPU: tests/screen_host.cpp runs it as a stand-alone program, built with -O2 and
again with the address and undefined-behaviour sanitizers (no preload, no Python, no GPU; the sequences sit in a heap block of exactly
their size).  Held, for equality, against tests/_screen_model.py; the library's own host-only entry points are held against the same."""
import math
import os
import struct
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import _screen_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILDS = {"O2": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover"]}


@pytest.fixture(scope="module", params=sorted(BUILDS))
def program(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("screen_" + request.param) / "screen_host")
    subprocess.check_call(["g++", "-std=c++17"] + BUILDS[request.param] + ["-I" + os.path.join(ROOT, "filtlong_amd", "csrc"), "-o", exe,
                                                                          os.path.join(ROOT, "tests", "screen_host.cpp")])
    return exe


def split(exe, tmp_path, seqs):
    src, dst = str(tmp_path / "seqs"), str(tmp_path / "pieces")
    with open(src, "wb") as f:
        f.write(struct.pack("<Q", len(seqs)))
        for s in seqs:
            f.write(struct.pack("<Q", len(s)) + bytes(s))
    p = subprocess.run([exe, "split", src, dst], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    blob = open(dst, "rb").read()
    n, = struct.unpack_from("<Q", blob, 0)
    assert len(blob) == 8 + 24 * n
    return [struct.unpack_from("<QQQ", blob, 8 + 24 * k) for k in range(n)]


def want_pieces(seqs):
    return [(i, a, b - a) for i, s in enumerate(seqs) for a, b in model.pieces(s)]


P_JUST_ABOVE_0 = (5e-324, 1e-300, 2.0 ** -40, 1e-9, 2.3283064365386963e-08)  # (the last: 100 / 2^32, where t = 1 exactly)


def test_threshold(program):
    for p in (100.0, 99.99999999999999, 10.0, 0.1, 1.0, 33.3, 50.0, 7.0, 60.0) + P_JUST_ABOVE_0:
        want = math.ceil(Fraction(p / 100.0) * (1 << 32))
        assert want == model.threshold(p)
        assert subprocess.check_output([program, "threshold", repr(p)]).decode().strip() == str(want), p
    assert model.threshold(100.0) == 1 << 32 and model.threshold(10.0) == 429496730
    assert model.threshold(1e-300) == 1  # a P above 0 asks for at least one hit in 2^32 windows ...
    assert model.threshold(5e-324) == 0  # ... unless P / 100 is no longer a double above 0: the definition is the IEEE quotient's
    for p in (0.0, -1.0, 100.00000000000001, 250.0, float("nan")):
        assert subprocess.check_output([program, "threshold", repr(p)]).decode().strip() == "invalid"


def test_library_threshold_and_span():
    """flx_screen_threshold / flx_screen_span are host only: they answer without a device"""
    from filtlong_amd import api
    for p in (100.0, 10.0, 0.1, 60.0) + P_JUST_ABOVE_0:
        assert api.screen_threshold(p) == math.ceil(Fraction(p / 100.0) * (1 << 32)), p
    for p in (0.0, -3.0, 100.5, float("nan")):
        with pytest.raises(api.FlxError) as e:
            api.screen_threshold(p)
        assert e.value.code == 1  # FLX_ERR_INVALID
    span = api.screen_span()
    assert span > 0 and span % 1024 == 0  # whole steps of the kernel
    # the decision on Python integers, at the edges of the comparison
    # (0.1 as a double lies above 1 / 10, and t is rounded up: 1 hit in 10 windows is below 10 %, 1 in 9 is not)
    hits, lengths = [1, 1, 0, 3, 0], [24, 25, 24, 35, 3]
    assert list(api.screen_excluded(hits, lengths, 10)) == [1, 0, 0, 1, 0] == [int(model.excluded(h, n, 10)) for h, n in zip(hits, lengths)]


def test_decision(program):
    rng = np.random.default_rng(3)
    cases = [(0, 0, 10.0), (0, 1, 10.0), (1, 10, 10.0), (1, 11, 10.0), (2**31 - 16, 2**31 - 16, 100.0), (2**31 - 17, 2**31 - 16, 100.0),
             (1, 2**31 - 16, 5e-324)]
    for _ in range(40):
        w = int(rng.integers(1, 1 << 31))
        cases.append((int(rng.integers(0, w + 1)), w, float(rng.choice([0.1, 10.0, 60.0, 100.0]))))
    for h, w, p in cases:
        t = model.threshold(p)
        want = w > 0 and (h << 32) >= t * w
        assert subprocess.check_output([program, "decide", str(h), str(w), str(t)]).decode().strip() == str(int(want)), (h, w, p)


def test_byte_classes(program, tmp_path):
    out = str(tmp_path / "bytes")
    subprocess.check_call([program, "bytes", out])
    got = open(out, "rb").read()
    want = bytearray(b"\xff" * 256)
    for i, c in enumerate(b"ACGT"):
        want[c] = want[c + 32] = i
    assert got == bytes(want)


def test_splitter(program, tmp_path):
    a16, a15 = b"ACGTACGTACGTACGT", b"ACGTACGTACGTACG"
    seqs = [
        a16 + b"N" + a16,                          # two pieces, one at either end
        b"N" + a16 + a16 + b"N",                   # one piece away from both ends
        a16 * 3,                                   # the whole sequence
        a15 + b"N" + a16,                          # a piece of 15 bases is dropped, one of 16 kept
        a16 + b"NNNNNNNNNNNNNNNNNNNNNNNN" + a15,    # a run of N, then 15: one piece
        b"NNNN" + a16.lower() + b"nn" + b"AcGt" * 5 + b"-",  # lowercase and mixed case are bases
        b"",                                       # an empty sequence
        b"N" * 40,                                 # nothing but N
        a15,                                       # shorter than a 16-mer
        a16 + b"R" + a16 + b"*" + a16 + b"\x00" + a16 + b"\xff" + a15,  # IUPAC codes, a NUL and 0xFF all cut
        b"",
        a16,                                       # the last sequence ends where the buffer ends
    ]
    got = split(program, tmp_path, seqs)
    assert got == want_pieces(seqs)
    assert [g for g in got if g[0] == 0] == [(0, 0, 16), (0, 17, 16)]
    assert [g for g in got if g[0] == 3] == [(3, 16, 16)]
    assert [g for g in got if g[0] == 4] == [(4, 0, 16)]
    assert [g for g in got if g[0] == 5] == [(5, 4, 16), (5, 22, 20)]
    assert not [g for g in got if g[0] in (6, 7, 8, 10)]
    assert split(program, tmp_path, []) == []
    assert split(program, tmp_path, [b""]) == []


def test_splitter_random(program, tmp_path):
    rng = np.random.default_rng(19)
    seqs = []
    for _ in range(60):
        n = int(rng.integers(0, 400))
        s = bytearray(model.random_seq(rng, n))
        for _ in range(int(rng.integers(0, 12))):
            if n:
                a, k = int(rng.integers(0, n)), int(rng.integers(1, 20))
                s[a:a + k] = bytes([int(rng.choice([78, 110, 0, 255, 45, 82]))]) * len(s[a:a + k])
        seqs.append(bytes(s))
    got = split(program, tmp_path, seqs)
    assert got == want_pieces(seqs) and len(got) > 60
