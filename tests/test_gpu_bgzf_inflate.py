"""BGZF members inflated on the GPU (flx_bgzf_inflate_dev, flx_bgzf_inflate): the corpus of tests/_bgzf_inflate_cases.py gives the
bytes and status words of the host walk of the same phases (tests/bgzf_inflate_host.cpp), member for member; first_bad; member
counts around the wave and the piece size; every alignment; compress -> inflate; the host-to-host object in pieces and from 16
threads.  The damaged members of the corpus pass the sanitizer build of tests/test_bgzf_inflate_host.py on the CPU."""
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import _bgzf
import _bgzf_inflate_cases as cases
from filtlong_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_fastq_ont  # noqa: E402

pytestmark = pytest.mark.gpu
PIECE = 4096  # members per piece of flx_bgzf_inflate (kInflatePiece in bgzf.hip)


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("inflate_corpus"))
    return cases.corpus(cases.build_host_encoder(d), d)


@pytest.fixture(scope="module")
def host_results(corpus, tmp_path_factory):
    d = tmp_path_factory.mktemp("inflate_host")
    exe = str(d / "bgzf_inflate_host")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I" + os.path.join(ROOT, "filtlong_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "bgzf_inflate_host.cpp")])
    cases.write_corpus(str(d / "corpus"), [c.member for c in corpus])
    subprocess.check_call([exe, str(d / "corpus"), str(d / "results")])
    return cases.read_results(str(d / "results"))


def inflate_dev(ctx, members, misalign=0):
    """-> ([(status, bytes)], first_bad); the output buffer is 0xAB where the kernel wrote nothing"""
    import torch
    n = len(members)
    blob = b"".join(members)
    in_off = np.concatenate([[0], np.cumsum([len(m) for m in members])]).astype(np.uint64)
    out_off = np.concatenate([[0], np.cumsum([cases.isize_of(m) for m in members])]).astype(np.uint64)
    d_in = torch.zeros(len(blob) + 32, dtype=torch.uint8, device="cuda")
    d_in[misalign:misalign + len(blob)] = torch.from_numpy(np.frombuffer(blob, dtype=np.uint8).copy()).to("cuda")
    d_io = torch.from_numpy(in_off.view(np.int64)).to("cuda")
    d_oo = torch.from_numpy(out_off.view(np.int64)).to("cuda")
    total = int(out_off[-1])
    d_out = torch.full((total + 32,), 0xAB, dtype=torch.uint8, device="cuda")
    d_st = torch.full((n + 1,), 0x7fffffff, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    fb = ctx.bgzf_inflate_dev(d_in.data_ptr() + misalign, d_io.data_ptr(), d_oo.data_ptr(), n, d_out.data_ptr() + misalign,
                              d_st.data_ptr())
    out = d_out.cpu().numpy()
    st = d_st.cpu().numpy()
    assert st[n] == 0x7fffffff and (out[:misalign] == 0xAB).all() and (out[misalign + total:] == 0xAB).all()
    o = out[misalign:].tobytes()
    return [(int(st[k]), o[int(out_off[k]):int(out_off[k + 1])]) for k in range(n)], fb


def test_corpus_equals_the_host_walk(ctx, corpus, host_results):
    got, fb = inflate_dev(ctx, [c.member for c in corpus])
    cases.check_results(corpus, got)
    for c, g, h in zip(corpus, got, host_results):
        assert g[0] == h[0], (c.name, g[0], h[0])
        if g[0] == 0:
            assert g[1] == h[1], c.name
        else:
            assert g[1] == b"\xab" * len(g[1]), c.name  # a member that is not ok leaves its range alone
    assert fb == next(k for k, g in enumerate(got) if g[0])


@pytest.mark.parametrize("where", ["first", "middle", "last", "none"])
def test_first_bad(ctx, where):
    good = cases.small_members(130)
    bad = cases.damaged_cases()
    members = [m for m, _ in good]
    at = {"first": [0, 77], "middle": [64, 65, 129], "last": [129], "none": []}[where]
    for k, i in enumerate(at):
        members[i] = bad[(3 * k + len(where)) % len(bad)].member
    got, fb = inflate_dev(ctx, members, misalign=3)
    assert fb == (at[0] if at else 130)
    for k, (st, b) in enumerate(got):
        assert (st != 0) == (k in at), k
        if k not in at:
            assert b == good[k][1], k  # the neighbours' bytes are right


@pytest.mark.parametrize("n", [1, 63, 64, 65, PIECE + 1])
def test_member_counts(ctx, n):
    ms = cases.small_members(n, seed=n)
    got, fb = inflate_dev(ctx, [m for m, _ in ms])
    assert fb == n and [g[1] for g in got] == [d for _, d in ms] and all(g[0] == 0 for g in got)
    z = api.Bgzf(ctx, slot_bytes=1 << 20, slots=2)
    try:
        assert z.inflate(b"".join(m for m, _ in ms)) == (b"".join(d for _, d in ms), n)
    finally:
        z.close()


def test_every_alignment(ctx):
    ms = cases.every_alignment()
    starts = np.cumsum([0] + [len(m) for m, _ in ms])[:-1]
    assert {int(s) % 16 for s in starts[::2]} == set(range(16))
    for mis in (0, 1):
        got, fb = inflate_dev(ctx, [m for m, _ in ms], misalign=mis)
        assert fb == len(ms) and [g[1] for g in got] == [d for _, d in ms]


def test_round_trip_and_the_object(ctx):
    data = gen_fastq_ont.generate(3 << 20, seed=12)
    z = api.Bgzf(ctx, slot_bytes=4 << 20, slots=4)
    small = api.Bgzf(ctx, slot_bytes=300000, slots=1)
    try:
        s = z.compress(data)
        n = len(api.bgzf_index(s)[0]) - 1
        assert n == -(-len(data) // _bgzf.MEMBER) + 1
        assert z.inflate(s) == (data, n)
        assert small.inflate(s) == (data, n)            # in slot-sized pieces: the same bytes
        assert z.inflate(b"") == (b"", 0)               # an empty call
        assert z.inflate(_bgzf.EOF_BLOCK) == (b"", 1)
        zl = _bgzf.zlib_bgzf(data, 6)
        assert small.inflate(zl) == (data, n)
        # a damaged member in the third piece: everything in front of it, and its index
        io = api.bgzf_index(zl)[0]
        bad = bytearray(zl)
        bad[int(io[20]) - 6] ^= 0x10                    # member 19's CRC-32
        assert small.inflate(bytes(bad)) == (data[:19 * _bgzf.MEMBER], 19)
        pieces = [_bgzf.zlib_bgzf(data[k * 150000:k * 150000 + 100000 + 9000 * k], 1 + k % 9, eof=bool(k & 1)) for k in range(16)]
        serial = [z.inflate(p) for p in pieces]
        for k, p in enumerate(pieces):
            assert serial[k][0] == data[k * 150000:k * 150000 + 100000 + 9000 * k]
        got = [None] * 16

        def work(k):
            got[k] = z.inflate(pieces[k])

        th = [threading.Thread(target=work, args=(k,)) for k in range(16)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        assert got == serial
    finally:
        z.close()
        small.close()


def test_timing_counts_launches(ctx):
    ms = cases.small_members(5)
    ctx.timing_enable(True)
    ctx.timing_reset()
    try:
        inflate_dev(ctx, [m for m, _ in ms])
        inflate_dev(ctx, [m for m, _ in ms])
        inflate_dev(ctx, [])
        ms_, launches = ctx.timing_get("flx_bgzf_inflate")
        assert launches == 2 and ms_ > 0
    finally:
        ctx.timing_enable(False)
