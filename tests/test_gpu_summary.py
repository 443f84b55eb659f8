"""flx_summary / flx_summary_dev (filtlong_amd/csrc/summary.hip) against the numpy restatement of tests/_summary.py: every field of
the struct, for equality, through the host-array and the device-pointer entry point — entry counts around the wave, the workgroup
and one sweep of the launched grid, masks, missing quality arrays, lengths that put all ten order statistics into one histogram
row or split them in the top or the bottom byte only, every length-bin boundary, sums beyond 2^32, qualities on, just below and
just above every exported edge — and with two and three ranks on one GPU over the loopback communicator."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _summary
from filtlong_amd import api

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
SHIM = os.path.join(HERE, "shim", "libloopback_rccl.so")
THREADS, MAX_BLOCKS = _summary.grid_constants()
SWEEP = THREADS * MAX_BLOCKS  # entries one pass of the full grid covers


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def edges():
    return api.summary_q_edges()


def check(ctx, edges, ln, mq=None, wq=None, mask=None):
    ln = np.ascontiguousarray(ln, dtype=np.int32)
    want = _summary.reference(ln, mq, wq, mask, edges)
    got = ctx.summary(ln, mq, wq, mask)
    assert not _summary.diff(got, want), ("flx_summary", _summary.diff(got, want))
    dev = [None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=t)).cuda()
           for a, t in ((ln, np.int32), (mq, np.float64), (wq, np.float64), (mask, np.uint8))]
    torch.cuda.synchronize()
    ptr = [None if d is None or d.numel() == 0 else d.data_ptr() for d in dev]
    got = ctx.summary_dev(len(ln), *ptr)
    assert not _summary.diff(got, want), ("flx_summary_dev", _summary.diff(got, want))
    return want


def random_case(rng, n):
    ln = rng.randint(0, 60000, n).astype(np.int32)
    mq = rng.uniform(0, 100, n)
    wq = mq * rng.uniform(0, 1, n)
    return ln, mq, wq


def test_exported_edges(edges):
    assert len(edges) == 51 and edges[0] == 0.0 and (np.diff(edges) > 0).all() and edges[50] < 100.0
    assert np.allclose(edges, 100.0 * (1.0 - 10.0 ** (-np.arange(51) / 10.0)), rtol=1e-15, atol=0)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, THREADS - 1, THREADS, THREADS + 1, SWEEP + 1])
def test_entry_counts(ctx, edges, n):
    rng = np.random.RandomState(n % 1000 + 1)
    ln, mq, wq = random_case(rng, n)
    want = check(ctx, edges, ln, mq, wq, (rng.uniform(0, 1, n) < 0.7).astype(np.uint8))
    assert want["n"] <= n
    assert check(ctx, edges, ln, mq, wq)["n"] == n


def test_masks_and_missing_qualities(ctx, edges):
    rng = np.random.RandomState(5)
    n = 3 * THREADS + 17
    ln, mq, wq = random_case(rng, n)
    one = np.zeros(n, np.uint8)
    one[n - 2] = 1
    for mask in (None, np.zeros(n, np.uint8), np.ones(n, np.uint8), (np.arange(n) % 2).astype(np.uint8), one, np.full(n, 255, np.uint8)):
        want = check(ctx, edges, ln, mq, wq, mask)
    assert check(ctx, edges, ln, mq, wq, np.zeros(n, np.uint8))["n"] == 0
    assert check(ctx, edges, ln, mq, wq, one)["nx"] == [int(ln[n - 2])] * 9
    for a, b in ((None, None), (mq, None), (None, wq)):
        want = check(ctx, edges, ln, a, b, one if a is None else None)
        assert sum(want["mean_q_count"]) == (0 if a is None else want["n"]) and sum(want["window_q_count"]) == (0 if b is None else want["n"])


LENGTH_SETS = {
    "all-equal": np.full(1000, 4242),
    "all-zero": np.zeros(300),
    "zero-and-one": np.array([0, 1, 1, 0, 0, 1, 0]),
    "top-byte": np.array([0x01000000, 0x7F000000] * 150 + [0x01000000]),
    "bottom-byte": np.array([0x00345601, 0x003456FE] * 150 + [0x003456FE]),
    "bin-edges": np.array(sorted({min(max((1 << b) + d, 0), 2 ** 31 - 1) for b in range(32) for d in (-1, 0, 1)})),
    "three-of-int-max": np.array([2 ** 31 - 1] * 3),
    "zeros-and-a-few": np.array([0] * 500 + [10, 1, 1]),
}


@pytest.mark.parametrize("name", sorted(LENGTH_SETS))
def test_lengths(ctx, edges, name):
    ln = LENGTH_SETS[name].astype(np.int64)
    rng = np.random.RandomState(len(ln))
    mq = rng.uniform(0, 100, len(ln))
    want = check(ctx, edges, ln, mq, mq * 0.5)
    check(ctx, edges, ln, mq, mq * 0.5, (np.arange(len(ln)) % 3 != 0).astype(np.uint8))
    if name == "three-of-int-max":
        assert want["bases"] == 3 * (2 ** 31 - 1) > 2 ** 32 and want["nx"] == [2 ** 31 - 1] * 9
    if name == "bin-edges":
        assert want["len_count"][0] == 2 and want["len_count"][1] == 2 and all(c == 3 for c in want["len_count"][2:31]) and want["len_count"][31] == 0
    if name == "all-equal":
        assert want["nx"] == [4242] * 9 and want["median_length"] == 4242


def test_negative_length_is_refused(ctx):
    with pytest.raises(api.FlxError):
        ctx.summary(np.array([5, -1, 7], dtype=np.int32))
    assert ctx.summary(np.array([5, -1, 7], dtype=np.int32), mask=np.array([1, 0, 1], np.uint8))["n"] == 2  # (not counted: not looked at)


def test_qualities_on_and_around_every_edge(ctx, edges):
    q = np.concatenate([edges, np.nextafter(edges, -np.inf), np.nextafter(edges, np.inf),
                        [0.0, -0.0, 100.0, np.nan, -1.0, -np.inf, np.inf, 1e-300, 99.9999999]])
    rng = np.random.RandomState(9)
    ln = rng.randint(1, 50000, len(q)).astype(np.int32)
    want = check(ctx, edges, ln, q, q[::-1].copy())
    # bin 51: the double below 0, NaN, -1, -inf; bin 50: edge 50, the double above it, 100, inf, 99.9999999; bin 0: edge 0, the double above
    # it, the double below edge 1, 0.0, -0.0, 1e-300; every bin between: its edge, the double above it, the double below the next edge
    assert want["mean_q_count"][51] == 4 and want["mean_q_count"][50] == 5
    assert want["mean_q_count"][0] == 6 and all(c == 3 for c in want["mean_q_count"][1:50])


def test_timing_bracket(ctx, edges):
    ln, mq, wq = random_case(np.random.RandomState(2), 5000)
    ctx.timing_enable(True)
    ctx.timing_reset()
    try:
        ctx.summary(ln, mq, wq)
        ms, launches = ctx.timing_get("flx_summary")
    finally:
        ctx.timing_enable(False)
        ctx.timing_reset()
    assert launches == 1 and ms > 0.0


RANK_CASES = [
    # name, n, world, block boundaries (uneven; one share empty)
    ("two", 5000, 2, [0, 1850, 5000]),
    ("two-one-empty", 700, 2, [0, 0, 700]),
    ("three-one-empty", 9001, 3, [0, 5400, 5400, 9001]),
    ("three-all-empty", 0, 3, [0, 0, 0, 0]),
]


@pytest.mark.parametrize("case", RANK_CASES, ids=[c[0] for c in RANK_CASES])
def test_ranks_on_one_gpu(tmp_path, ctx, edges, case):
    name, n, world, bounds = case
    subprocess.check_call(["make", "-s", "-C", os.path.join(HERE, "shim")])
    rng = np.random.RandomState(n + world)
    ln, mq, wq = random_case(rng, n)
    if n:
        ln[: n // 3] = 0x00A00000 + rng.randint(0, 3, n // 3)  # few distinct long lengths: targets share rows across the ranks
    mask = (rng.uniform(0, 1, n) < 0.8).astype(np.uint8)
    work = str(tmp_path)
    np.savez(os.path.join(work, name + ".npz"), length=ln, mean=mq, window=wq, mask=mask, bounds=np.array(bounds, dtype=np.int64))
    env = dict(os.environ, FLX_RCCL_LIB=SHIM)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "_summary_worker.py"), str(r), str(world), work, name], env=env,
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE) for r in range(world)]
    outs = [p.communicate(timeout=300) for p in procs]
    for r, (p, (so, se)) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, "rank %d: %s" % (r, se.decode()[-2000:])
    whole = check(ctx, edges, ln, mq, wq, mask)
    whole_plain = _summary.reference(ln, None, None, None, edges)
    for r in range(world):
        got = json.load(open(os.path.join(work, "%s.out%d.json" % (name, r))))
        lo, hi = bounds[r], bounds[r + 1]
        assert not _summary.diff(got["global"], whole), (r, _summary.diff(got["global"], whole))
        assert not _summary.diff(got["global_dev"], whole), (r, _summary.diff(got["global_dev"], whole))
        assert not _summary.diff(got["global_lengths_only"], whole_plain), r
        local = _summary.reference(ln[lo:hi], mq[lo:hi], wq[lo:hi], mask[lo:hi], edges)
        assert not _summary.diff(got["local"], local), (r, _summary.diff(got["local"], local))
