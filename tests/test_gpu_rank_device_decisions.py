"""flx_rank_and_cut_dev with the stage's decisions taken on the device (rank.hip: cut_by_select, the record filled by the
sequence itself): every outcome of the cut, on device arrays, against the oracle — pass flags, report fields, final scores.  Where
the single-wait sequence is expected to have served the call (no redo with host values), the timing brackets say so: it never launches the separate passed-bases kernel."""
import os

import numpy as np
import pytest

import _oracle
from filtlong_amd import api

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    for k in ("FLX_RANK_SORT", "FLX_RANK_EXACT"):
        os.environ.pop(k, None)
    c = api.Context(0)
    yield c
    c.close()


def reads2(n, seed):
    rng = np.random.RandomState(seed)
    mean = rng.uniform(60, 99, n)
    window = mean * rng.uniform(0.3, 1.05, n)
    length = np.clip(rng.gamma(4, 2500, n), 1, None).astype(np.int32)
    passed = (rng.random_sample(n) > 0.1).astype(np.uint8)
    return mean, window, length, passed


def run_dev(ctx, mean, window, length, passed, device_path=None, scores=True, **kw):
    """One call on device arrays, compared with the oracle.  device_path: True / False = the call must (not) have been served by the
    single-wait sequence; None = not checked.  scores=False: the final scores are not compared (the forced host cut never wrote them)."""
    import torch
    n = len(mean)
    want = _oracle.rank_and_cut(mean, window, length, passed, **kw)
    d = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (mean.astype(np.float64), window.astype(np.float64),
                                                                  length.astype(np.int32), passed.astype(np.uint8).copy())]
    d_fs = torch.full((max(n, 1),), -1.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    total = kw.get("total_bases")
    if total is None:
        total = int(length.astype(np.int64).sum())
    ctx.timing_enable(True)
    ctx.timing_reset()
    rep = ctx.rank_and_cut_dev(n, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(),
                               length_weight=kw.get("lw", 1.0), mean_q_weight=kw.get("mw", 1.0), window_q_weight=kw.get("ww", 1.0),
                               target_bases=kw.get("target_bases"), keep_percent=kw.get("keep_percent"), total_bases=total,
                               d_final_score=d_fs.data_ptr())
    host_driven = ctx.timing_get("flx_rank_passed_bases")[1]
    selects = ctx.timing_get("flx_rank_select")[1]
    ctx.timing_enable(False)
    torch.cuda.synchronize()
    got = d[3].cpu().numpy()
    assert rep.outcome == want["outcome"]
    assert rep.target_bases == want["target_bases"]
    assert (got == want["passed"]).all(), "pass set differs (%d reads)" % int((got != want["passed"]).sum())
    if want["outcome"] == 3:
        assert rep.kept_bases == want["kept_bases"]
    for a, b in ((rep.mean_quality, want["mean_quality"]), (rep.stdev_quality, want["stdev_quality"]),
                 (rep.min_z, want["min_z"]), (rep.max_z, want["max_z"])):
        assert a == b or (np.isnan(a) and np.isnan(b))
    if n and scores:
        fs, wf = d_fs.cpu().numpy()[:n], want["final_score"]
        ok = ~np.isnan(wf)
        assert np.allclose(fs[ok], wf[ok], rtol=1e-12, atol=0)
    if device_path is True:
        assert host_driven == 0 and selects == 1, "the call went through the host-driven sequence"
    elif device_path is False:
        assert selects == 0 or host_driven > 0
    return rep


@pytest.mark.parametrize("n,seed", [(2, 2), (65, 3), (1000, 4), (4097, 5), (100_000, 6), (1_000_000, 7)])
def test_sorted(ctx, n, seed):
    mean, window, length, passed = reads2(n, seed)
    tot = int(length.astype(np.int64).sum())
    for frac in (0.01, 0.33, 0.5, 0.9, 0.999):
        rep = run_dev(ctx, mean, window, length, passed, device_path=True, target_bases=max(1, int(tot * frac)))
        assert rep.outcome != 3 or rep.exact_fallback == 0
    run_dev(ctx, mean, window, length, passed, device_path=True, keep_percent=42.5)
    run_dev(ctx, mean, window, length, passed, device_path=True, keep_percent=80.0, target_bases=tot // 3, lw=2.0, mw=0.5, ww=3.0)


def test_not_enough_and_no_cut(ctx):
    mean, window, length, passed = reads2(5000, 8)
    tot = int(length.astype(np.int64).sum())
    assert run_dev(ctx, mean, window, length, passed, target_bases=tot).outcome == 1
    assert run_dev(ctx, mean, window, length, passed, target_bases=tot + 12345).outcome == 1
    assert run_dev(ctx, mean, window, length, passed).outcome == 0


def test_already_below(ctx):
    """target < total bases but >= the bases that passed the hard cut-offs: found on the device (the first histogram's total),
    the flags stay as they were and the final scores are still written."""
    mean, window, length, passed = reads2(20_000, 9)
    tot = int(length.astype(np.int64).sum())
    pb = int(length[passed != 0].astype(np.int64).sum())
    assert pb < tot - 1
    for target in (pb, pb + 1, tot - 1):
        assert run_dev(ctx, mean, window, length, passed, device_path=True, target_bases=target, total_bases=tot).outcome == 2
    assert run_dev(ctx, mean, window, length, passed, device_path=True, target_bases=pb - 1, total_bases=tot).outcome == 3


def test_nan_scores(ctx):
    """stdev == 0 -> 0/0 (main.cpp:192-195,206): every score NaN; the reference's own order on the host."""
    n = 500
    rng = np.random.RandomState(3)
    length = rng.randint(100, 5000, n).astype(np.int32)
    rep = run_dev(ctx, np.full(n, 77.0), np.full(n, 70.0), length, np.ones(n, np.uint8), device_path=True,
                  target_bases=int(length.sum()) // 2)
    assert rep.exact_fallback == 1


def test_real_tie_group_straddling_the_cut(ctx):
    """Exact duplicates tie exactly; where such a group straddles the cut only the reference's std::sort can decide and the audit
    must hand over to it."""
    rng = np.random.RandomState(21)
    n = 3000
    mean, window, length, passed = reads2(n, 21)
    src, dst = rng.randint(0, n, 2500), rng.randint(0, n, 2500)
    mean[dst], window[dst], length[dst] = mean[src], window[src], length[src]
    tot = int(length.astype(np.int64).sum())
    fallbacks = 0
    for t in np.linspace(tot * 0.05, tot * 0.95, 40):
        fallbacks += run_dev(ctx, mean, window, length, passed, device_path=True, target_bases=int(t)).exact_fallback
    assert fallbacks > 0


def test_forced_exact_path(ctx):
    mean, window, length, passed = reads2(30_000, 22)
    tot = int(length.astype(np.int64).sum())
    os.environ["FLX_RANK_EXACT"] = "1"
    try:
        rep = run_dev(ctx, mean, window, length, passed, device_path=False, scores=False, target_bases=tot // 2)
    finally:
        os.environ.pop("FLX_RANK_EXACT", None)
    assert rep.exact_fallback == 1


def test_band_larger_than_capacity(ctx):
    """More equal scores around the cut than the select path audits (2^16): the sort path takes over, same result."""
    n = 200_000
    mean, window, length, passed = reads2(n, 23)
    rng = np.random.RandomState(24)
    dup = rng.choice(n, 70_000, replace=False)
    order = np.argsort(mean)
    mid = order[n // 2]
    mean[dup], window[dup], length[dup] = mean[mid], window[mid], length[mid]
    passed[dup] = 1
    tot = int(length.astype(np.int64).sum())
    # a target inside the group of duplicates: bases of the passed reads that score better, plus a part of the group
    want_all = _oracle.rank_and_cut(mean, window, length, passed, target_bases=tot)  # (scores only)
    fs = want_all["final_score"]
    better = int(length[(fs > fs[mid]) & (passed != 0)].astype(np.int64).sum())
    target = better + int(length[mid]) * 30_000 + 1
    rep = run_dev(ctx, mean, window, length, passed, device_path=True, target_bases=target)
    assert rep.outcome == 3
    # and a band between what comes back with the record (1024) and the capacity: the second round trip of the select path.  Equal
    # lengths and a target that only the group's LAST member reaches keep the whole group in any order: no fallback, the gathered
    # records themselves are audited
    mean, window, length, passed = reads2(n, 25)
    dup = rng.choice(n, 5000, replace=False)
    mid = np.argsort(mean)[n // 2]
    mean[dup], window[dup], length[dup] = mean[mid], window[mid], length[mid]
    passed[dup] = 1
    passed[mid] = 1
    m = len(set(dup.tolist()) | {int(mid)})
    tot = int(length.astype(np.int64).sum())
    fs = _oracle.rank_and_cut(mean, window, length, passed, target_bases=tot)["final_score"]
    better = int(length[(fs > fs[mid]) & (passed != 0)].astype(np.int64).sum())
    rep = run_dev(ctx, mean, window, length, passed, device_path=True, target_bases=better + int(length[mid]) * (m - 1) + 1)
    assert rep.outcome == 3 and rep.exact_fallback == 0 and rep.audited >= m > 1024


def test_empty_and_single(ctx):
    e = np.zeros(0)
    rep = run_dev(ctx, e, e, np.zeros(0, np.int32), np.zeros(0, np.uint8), target_bases=100, total_bases=0)
    assert rep.outcome == 1
    one = (np.array([88.0]), np.array([80.0]), np.array([5000], np.int32))
    assert run_dev(ctx, *one, np.array([1], np.uint8), device_path=True, target_bases=1).outcome == 3
    assert run_dev(ctx, *one, np.array([0], np.uint8), device_path=True, target_bases=1, total_bases=5000).outcome == 2


def test_repeated_calls_reuse_the_buffers(ctx):
    """Calls of different sizes back to back on one context: the record, the band and the pinned buffer are reused."""
    for n, seed in ((70_000, 31), (300, 32), (250_000, 33), (300, 32)):
        mean, window, length, passed = reads2(n, seed)
        tot = int(length.astype(np.int64).sum())
        run_dev(ctx, mean, window, length, passed, device_path=True, target_bases=tot // 2)
