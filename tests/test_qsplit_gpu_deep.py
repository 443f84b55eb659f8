"""--split_window_q on the GPU where the window is deeper than one wave step and where the quality bytes are any byte at all.

k_qsplit_detect walks a read 1024 bases a step and fetches the trailing edge of the window n - 1 bases back: with W = 2048 .. 20 000
that edge lies 2 .. 20 steps behind, the carry holds a window sum across many steps, the first whole steps have no window and no
trailing byte, and n = L spans several steps.  The table has 256 rows, bytes from 128 on are signed in the definition, and on the GPU
such bytes also reach the children's scoring call over a plane that k_qsplit_gather built.  Everything is compared for equality with
the model of tests/_qsplit_model.py, the library without the flag, flx_score_batch over the children's substrings and the oracle
(check_split of tests/test_qsplit_gpu.py); every (W, Q) asserts on the model, before the library is called, that its input holds a
read that splits, a wholly bad read and an untouched one."""
import ctypes as C

import numpy as np
import pytest

import _qsplit_model as model
from filtlong_amd import api
from test_qsplit_gpu import PHRED, STEP, Batch, check_split, same_scores

pytestmark = pytest.mark.gpu
DEEP_W = (1026, 2047, 2048, 2049, 3000, 3 * STEP + 7, 5000, 20000)
FIELDS = ("child_offsets", "child_ranges", "first", "last", "passed", "child_passed")


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


def any_byte_read(rng, length, w):
    """Phred 30-93 with W / 2 junk bases in the middle, then max(4, L / 200) positions overwritten with bytes drawn from 0..255;
    the bytes 127 and 128 (the edge of the signed definition, and a byte >= 128) and a byte below '!' are placed where the draw
    misses them."""
    s = bytearray(model.junk_read(rng, length, [(length // 2, length // 2 + w // 2)], good=(30, 93), junk=PHRED["junk"]))
    at = rng.choice(length, size=max(4, length // 200), replace=False)
    drawn = [int(b) for b in rng.integers(0, 256, size=len(at))]
    for k, (need, fill) in enumerate(((lambda b: b == 127, 127), (lambda b: b == 128, 128), (lambda b: b < 33, 10), (lambda b: b >= 128, 255))):
        if not any(need(b) for b in drawn):
            drawn[k] = fill
    for p, b in zip(at, drawn):
        s[int(p)] = b
    assert 127 in drawn and 128 in drawn and min(drawn) < 33 and max(drawn) >= 128
    return bytes(s)


def deep_reads(w):
    """220 reads per window size: lengths on both sides of W, 2 W and the wave step; no junk, all junk, one junk stretch at the
    window's and the read's edges; two reads of any byte."""
    rng = np.random.default_rng(1000 + w)
    quals = []
    for length in (w - 1, w, w + 1, w + 16, 2 * w - 1, 2 * w, 2 * w + 1, 3 * w + 7, (2 * w // STEP + 1) * STEP, (3 * w // STEP + 1) * STEP + 1):
        quals.append(model.junk_read(rng, length, [], **PHRED))
        quals.append(model.junk_read(rng, length, [(0, length)], **PHRED))
        for at in (0, w // 2, w - 1, w, length - w, length - w // 2 - 1, length // 2):
            for n in (w // 4 + 1, w // 2, w):
                if 0 <= at < length:
                    quals.append(model.junk_read(rng, length, [(at, at + n)], **PHRED))
    quals.append(any_byte_read(rng, w + 1, w))
    quals.append(any_byte_read(rng, 3 * w + 7, w))
    return quals


_batches = {}


def deep_batch(w):
    if w not in _batches:
        _batches[w] = Batch(deep_reads(w))
        assert len(_batches[w].quals) == 220
    return _batches[w]


def model_census(batch, w, q):
    """The condition on the input, on the model alone: a read that splits, a wholly bad read, an untouched read."""
    off, _, _, _, wholly = model.split_batch(batch.quals, w, q)
    census = model.census(off, wholly)
    assert min(census) > 0, "W=%d Q=%g: (split, wholly bad, untouched) = %r" % (w, q, census)
    return off


def check_child_bytes(got, lengths):
    """What no right answer can be: a pass flag that is neither 0 nor 1, a range outside its read or empty, ranges of one parent that
    touch or go back (the device outputs start out as 0xA5 bytes: a child the kernels did not write fails here)."""
    off, rng = got["child_offsets"].astype(np.int64), got["child_ranges"].astype(np.int64)
    assert off[0] == 0 and (np.diff(off) >= 0).all() and off[-1] == len(rng) == len(got["child_passed"])
    assert np.isin(got["child_passed"], (0, 1)).all() and np.isin(got["passed"], (0, 1)).all()
    parent = np.repeat(np.arange(len(lengths)), np.diff(off))
    assert (rng[:, 0] >= 0).all() and (rng[:, 1] <= np.asarray(lengths, dtype=np.int64)[parent]).all() and (rng[:, 0] < rng[:, 1]).all()
    same = parent[1:] == parent[:-1]
    assert (rng[1:, 0][same] > rng[:-1, 1][same]).all(), "children of one read at least one base apart, in increasing order"


def same_result(got, want, what):
    for key in FIELDS:
        assert got[key].shape == want[key].shape and (got[key] == want[key]).all(), (what, key)
    same_scores((got["mean_q"], got["window_q"], got["passed"]), (want["mean_q"], want["window_q"], want["passed"]), what + " parents")
    same_scores((got["child_mean_q"], got["child_window_q"], got["child_passed"]),
                (want["child_mean_q"], want["child_window_q"], want["child_passed"]), what + " children")


@pytest.mark.parametrize("q", [50, 85, 99])
@pytest.mark.parametrize("w", DEEP_W)
def test_deep_windows_against_the_model(ctx, w, q):
    batch = deep_batch(w)
    off = model_census(batch, w, q)
    got, _ = check_split(ctx, batch, w, q)
    check_child_bytes(got, batch.lengths)
    assert int(off[-1]) == len(got["child_ranges"])


@pytest.mark.parametrize("w", DEEP_W)
def test_no_order_is_the_same_result(ctx, w):
    """Every other call of the path passes a length order; without one the reads and the children come out the same."""
    batch = deep_batch(w)
    model_census(batch, w, 85)
    p = api.make_params(window_size=w)
    ordered = ctx.score_reads(batch.plane, batch.offsets, batch.lengths, p, order=batch.order, split_window_q=85)
    plain = ctx.score_reads(batch.plane, batch.offsets, batch.lengths, p, order=None, split_window_q=85)
    check_child_bytes(plain, batch.lengths)
    same_result(plain, ordered, "W=%d without an order" % w)


@pytest.fixture(scope="module")
def byte_batch():
    """Any byte at ordinary windows: 300 reads of 0..5000 uniformly random bytes (nearly all wholly bad: they are here for the
    table's rows), 50 reads of Phred 30-93 with 1 % of their bytes random (the even ones scattered, the odd ones in one burst in
    the read's second quarter, which is what spoils a window of 250 at Q = 85), and every byte in rising and in falling order."""
    rng = np.random.default_rng(256)
    quals = [rng.integers(0, 256, size=int(rng.integers(0, 5001))).astype(np.uint8).tobytes() for _ in range(300)]
    mostly_good = []
    for i in range(50):
        length = int(rng.integers(8000, 12001))
        s = np.frombuffer(model.junk_read(rng, length, [], good=(30, 93)), dtype=np.uint8).copy()
        k = length // 100
        at = rng.choice(length, size=k, replace=False) if i % 2 == 0 else int(rng.integers(length // 4, length // 2)) + np.arange(k)
        s[at] = rng.integers(0, 256, size=k)
        mostly_good.append(s.tobytes())
    every = bytes(range(256)) * 8
    return Batch(quals + mostly_good + [every, every[::-1]]), mostly_good


@pytest.mark.parametrize("tables", [None, "plain", "private"])
@pytest.mark.parametrize("w,q", [(1, 85), (7, 50), (250, 85), (250, 99), (1000, 99)])
def test_any_byte_at_ordinary_windows(ctx, byte_batch, monkeypatch, w, q, tables):
    batch, mostly_good = byte_batch
    off, _, _, _, wholly = model.split_batch(mostly_good, w, q)
    assert model.census(off, wholly)[0] > 0, "no mostly good read splits at W=%d Q=%g" % (w, q)
    if tables is None:
        monkeypatch.delenv("FLX_PHRED_TABLES", raising=False)
    else:
        monkeypatch.setenv("FLX_PHRED_TABLES", tables)
    got, _ = check_split(ctx, batch, w, q, expect=("split",))
    check_child_bytes(got, batch.lengths)


def test_exact_capacity_and_no_first_last(ctx):
    """child_capacity == the number of children succeeds, one less is FLX_ERR_CAPACITY with the number in n_children, and a call
    without first / last (the library's own scratch arrays stand in) gives the same children."""
    w, q = 3000, 85
    batch = deep_batch(w)
    off = model_census(batch, w, q)
    want, _ = check_split(ctx, batch, w, q)
    n, nc = len(batch.quals), int(off[-1])

    def call(capacity, with_first_last):
        a = dict(mean_q=np.zeros(n, np.float64), window_q=np.zeros(n, np.float64), passed=np.zeros(n, np.uint8),
                 first=np.full(n, -7, np.int32), last=np.full(n, -7, np.int32), child_offsets=np.zeros(n + 1, np.uint64),
                 child_ranges=np.zeros(2 * capacity, np.int32), child_mean_q=np.zeros(capacity, np.float64),
                 child_window_q=np.zeros(capacity, np.float64), child_passed=np.zeros(capacity, np.uint8))
        s = api.Scores()
        for key, arr in a.items():
            if with_first_last or key not in ("first", "last"):
                setattr(s, key, arr.ctypes.data)
        s.child_capacity = capacity
        rc = ctx.L.flx_score_batch_qsplit(ctx.h, batch.plane.ctypes.data, batch.plane.nbytes, batch.offsets.ctypes.data, batch.lengths.ctypes.data,
                                          batch.order.ctypes.data, n, C.byref(api.make_params(window_size=w)), float(q), C.byref(s))
        a["child_ranges"] = a["child_ranges"].reshape(-1, 2)
        return rc, int(s.n_children), a

    rc, got_nc, exact = call(nc, True)
    assert rc == 0 and got_nc == nc
    same_result(exact, want, "capacity == children")
    rc, got_nc, _ = call(nc - 1, True)
    assert rc == 5 and got_nc == nc
    rc, got_nc, bare = call(nc, False)
    assert rc == 0 and got_nc == nc
    assert (bare["first"] == -7).all() and (bare["last"] == -7).all()  # (not asked for: not written)
    bare["first"], bare["last"] = want["first"], want["last"]
    same_result(bare, want, "without first / last")
    check_child_bytes(bare, batch.lengths)


@pytest.mark.parametrize("w", [3000, 5000])
def test_deep_windows_through_the_pipeline(ctx, w):
    """The same reads through flx_pipeline_* in chunks of 37 reads; a chunk larger than the slots makes them grow."""
    batch = deep_batch(w)
    model_census(batch, w, 85)
    one, _ = check_split(ctx, batch, w, 85)
    chunks = [batch.quals[i:i + 37] for i in range(0, len(batch.quals), 37)]
    got = ctx.score_stream(chunks, api.make_params(window_size=w), chunk_bytes=1 << 18, chunk_reads=64, grow=True, split_window_q=85)
    same_result(got, one, "W=%d pipeline" % w)
    check_child_bytes(got, batch.lengths)


def test_long_children_at_a_deep_window(ctx, monkeypatch):
    """300 000 bases, junk stretches of 6000 bases across step boundaries, W = 5000: the trailing edge is five steps back for 290
    steps, and with FLX_PHRED_LONG_MIN=4096 the children take the cooperative path."""
    monkeypatch.setenv("FLX_PHRED_LONG_MIN", "4096")
    rng = np.random.default_rng(53)
    st = [(k * STEP - 40, k * STEP - 40 + 6000) for k in (20, 100, 101, 200)] + [(0, 10), (299_900, 300_000)]
    batch = Batch([model.junk_read(rng, 300_000, st, **PHRED), model.junk_read(rng, 16_000, [(6000, 12_000)], **PHRED), b"~" * 100])
    off, _, _, _, wholly = model.split_batch(batch.quals, 5000, 85)
    assert model.census(off, wholly)[0] > 0 and model.census(off, wholly)[2] > 0
    ctx.timing_enable(True)
    ctx.timing_reset()
    got, _ = check_split(ctx, batch, 5000, 85, expect=("split", "untouched"))
    long_launches = ctx.timing_get("flx_score_phred_long")[1]
    ctx.timing_enable(False)
    check_child_bytes(got, batch.lengths)
    assert (got["child_ranges"][:, 1] - got["child_ranges"][:, 0]).max() > 4096 and long_launches > 0
