"""BGZF compression on the GPU (flx_bgzf_compress_dev, flx_bgzf): every output round-trips exactly through the strict
validator of tests/_bgzf.py; sizes against zlib on the same 65280-byte grid; determinism; the capacity error."""
import os
import random
import sys
import threading

import numpy as np
import pytest

import _bgzf
from filtlong_amd import api
from filtlong_amd._lib import FlxError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_fastq_ont  # noqa: E402

pytestmark = pytest.mark.gpu
M = _bgzf.MEMBER


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ont():
    return gen_fastq_ont.generate(24 << 20, seed=7)


def compress(ctx, data, eof=True, misalign=0):
    import torch
    n = len(data)
    d_in = torch.empty(n + 16, dtype=torch.uint8, device="cuda")
    if n:
        d_in[misalign:misalign + n] = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to("cuda")
    cap = api.bgzf_bound(n, eof)
    d_out = torch.empty(max(cap, 1), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    got = ctx.bgzf_compress_dev(d_in.data_ptr() + misalign, n, d_out.data_ptr(), cap, eof=eof)
    assert got <= cap
    return d_out[:got].cpu().numpy().tobytes()


def check(ctx, data, eof=True, **kw):
    s = compress(ctx, data, eof=eof, **kw)
    got, info = _bgzf.validate(s, require_eof=eof)
    assert got == data
    assert [m[2] for m in info["members"] if m[2]] == [min(M, len(data) - k) for k in range(0, len(data), M)]
    for _, size, isize in info["members"]:
        assert size <= isize + 5 + 26 or isize == 0  # never beyond a stored block plus the member's 26 bytes
    assert len(s) <= api.bgzf_bound(len(data), eof)
    return s


def test_empty(ctx):
    assert compress(ctx, b"", eof=True) == _bgzf.EOF_BLOCK
    assert compress(ctx, b"", eof=False) == b""


@pytest.mark.parametrize("n", [1, 65279, 65280, 65281, 3 * 65280 + 17])
def test_sizes_around_the_member(ctx, ont, n):
    check(ctx, ont[:n])
    check(ctx, ont[:n], eof=False)


def test_hundred_million_bytes(ctx, ont):
    r = np.random.default_rng(3)
    data = (ont * 5)[:10 ** 8]
    data = data[:40 << 20] + r.integers(0, 256, 4 << 20, dtype=np.uint8).tobytes() + data[44 << 20:]
    check(ctx, data)


def test_random_sizes(ctx, ont):
    r = random.Random(2026)
    for _ in range(200):
        n = r.randrange(0, 3 << 20)
        at = r.randrange(0, len(ont) - n)
        check(ctx, ont[at:at + n], eof=r.random() < 0.5, misalign=r.choice((0, 0, 1, 3, 8)))


def test_byte_values_random_and_runs(ctx):
    check(ctx, bytes(range(256)))
    rnd = np.random.default_rng(9).integers(0, 256, 5 << 20, dtype=np.uint8).tobytes()
    s = check(ctx, rnd)
    members = -(-len(rnd) // M)
    assert len(s) <= len(rnd) + 31 * members + 28
    for n in (257, 258, 259, 260, 516, 517, 65280, 300000):
        check(ctx, b"\xee" * n)
        check(ctx, b"ab" + b"\x00" * n + b"cd")


@pytest.mark.parametrize("period", [1, 2, 3, 4, 257, 32767, 32768, 32769, 40000])
def test_periodic(ctx, period):
    base = np.random.default_rng(period).integers(0, 256, period, dtype=np.uint8).tobytes()
    data = (base * (400000 // period + 2))[:400000]
    s = check(ctx, data)
    if period <= 32768:  # the repeats are found (a member's first period has nothing to match)
        assert len(s) < (len(data) // 20 if period <= 257 else len(data) * 3 // 4)
    if period > 32768:
        assert len(s) > len(data)  # nothing within reach: stored


def test_match_in_the_previous_member(ctx):
    x = np.random.default_rng(4).integers(0, 256, M, dtype=np.uint8).tobytes()
    check(ctx, x + x[-5000:] + x[:3000])


def test_fibonacci_frequencies(ctx):
    fib = [1, 1]
    while len(fib) < 26:
        fib.append(fib[-1] + fib[-2])
    syms = np.repeat(np.arange(26, dtype=np.uint8), np.minimum(fib, 40000))
    np.random.default_rng(1).shuffle(syms)
    check(ctx, syms.tobytes())


def test_ont_size_against_zlib(ctx, ont):
    s = check(ctx, ont)
    z1 = len(_bgzf.zlib_bgzf(ont, 1))
    assert len(s) <= 1.10 * z1, (len(s), z1)


def test_same_bytes_as_the_host_encoder(ctx, ont, tmp_path):
    import subprocess
    exe = str(tmp_path / "bgzf_host")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "filtlong_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "bgzf_host.cpp")])
    data = ont[:1 << 20] + bytes(range(256)) * 300
    (tmp_path / "in").write_bytes(data)
    subprocess.check_call([exe, str(tmp_path / "in"), str(tmp_path / "out")])
    assert compress(ctx, data) == (tmp_path / "out").read_bytes()


def test_deterministic_and_thread_safe(ctx, ont):
    data = ont[:20 << 20]
    a = compress(ctx, data)
    assert compress(ctx, data) == a
    z = api.Bgzf(ctx, slot_bytes=4 << 20, slots=4)
    try:
        assert z.compress(data) == a  # in slot-sized pieces: the same bytes
        pieces = [ont[k << 20:(k << 20) + (1 << 20) + 1000 * k] for k in range(16)]
        serial = [z.compress(p, eof=bool(k & 1)) for k, p in enumerate(pieces)]
        for k, p in enumerate(pieces):
            assert _bgzf.validate(serial[k], require_eof=bool(k & 1))[0] == p
        got = [None] * 16

        def work(k):
            got[k] = z.compress(pieces[k], eof=bool(k & 1))

        th = [threading.Thread(target=work, args=(k,)) for k in range(16)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        assert got == serial
        assert z.compress(b"") == _bgzf.EOF_BLOCK
        with pytest.raises(FlxError) as e:
            z.compress(data, out_cap=len(a) - 1)
        assert e.value.code == 5
    finally:
        z.close()


def test_capacity_and_timing(ctx, ont):
    import torch
    data = ont[:1 << 20]
    s = compress(ctx, data)
    d_in = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to("cuda")
    d_out = torch.zeros(len(s), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    with pytest.raises(FlxError) as e:
        ctx.bgzf_compress_dev(d_in.data_ptr(), len(data), d_out.data_ptr(), len(s) - 1)
    assert e.value.code == 5
    with pytest.raises(FlxError) as e:  # room for the members, not for the end-of-file block
        ctx.bgzf_compress_dev(d_in.data_ptr(), len(data), d_out.data_ptr(), len(s) - 28)
    assert e.value.code == 5
    ctx.timing_enable(True)
    ctx.timing_reset()
    try:
        assert ctx.bgzf_compress_dev(d_in.data_ptr(), len(data), d_out.data_ptr(), len(s)) == len(s)
        ms, launches = ctx.timing_get("flx_bgzf")
        assert launches == 1 and ms > 0
    finally:
        ctx.timing_enable(False)
    assert d_out.cpu().numpy().tobytes() == s
