"""flx_complexity_bad at the edges of its LAUNCH GEOMETRY, against tests/_complexity_model.py (bad_many) for equality.

k_complexity_bad (csrc/complexity.hip) is persistent: 8 workgroups of 4 waves per CU walk the spans with `sp += n_waves`; a span is
complexity_span() window start positions of one read and every lane of a wave owns span / 64 consecutive ones (its RUN), walking
run + 63 bases from a fresh state; in the last span of a read the run is a 64th of the windows left, rounded up to a multiple of 16
(csrc/complexity.h: lane_run).  So the edges are the run (where one lane's windows end and the next lane's begin), the run plus the
63 bases of warm-up, the span (where the next wave begins) and the span plus warm-up — all taken from complexity_span() and
complexity_window(), none a literal — and, for the shorter runs, the numbers of windows at which the run grows by 16.

  the edges    one read per length around every edge, each with a repeat island that straddles exactly that edge (and one that ends on
               it, and one that begins on it): a window counted twice, or by nobody, moves the count
  the crowd    more than twice the short reads of one pass of the grid's waves (sized from device_info()["n_cu"]), so every wave comes round
               `sp += n_waves` a second time: a second binary search, a second clearing of the counters in LDS, a second atomicAdd
               by the same wave; reads below 64 bases (no span) among them, and two reads of several spans at the start and the end

each with order NULL, the length order and a random permutation."""
import numpy as np
import pytest

import _complexity_cases as cases
import _complexity_model as model
from filtlong_amd import api

pytestmark = pytest.mark.gpu
WAVES_PER_CU = 8 * 4  # csrc/complexity.hip: kComplexityBlocksPerCU workgroups of kComplexityThreads / 64 waves


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


def orders(lengths, seed):
    return (None, api.length_order(lengths), np.random.default_rng(seed).permutation(len(lengths)).astype(np.uint32))


def check(ctx, reads, T=20):
    plane, offsets, lengths = api.pack_reads(reads)
    want = model.bad_many(reads, T)
    for order in orders(lengths, len(reads)):
        got = ctx.complexity_bad(plane, offsets, lengths, score=T, order=order)
        bad = np.flatnonzero(got != want)
        assert len(bad) == 0, (order is None, len(bad), [(int(i), len(reads[i]), int(got[i]), int(want[i])) for i in bad[:10]])
    return want


def test_edges(ctx):
    window, span = api.complexity_window(), api.complexity_span()
    run, warm = span // 64, window - 1
    rng = np.random.default_rng(9)
    reads = []
    for edge in (run, run + warm, 2 * run, 63 * run, 63 * run + warm, span, span + warm, span + run, 2 * span, 2 * span + warm):
        for length in (edge + warm - 1, edge + warm, edge + warm + 1, edge + warm + window, edge + warm + run + 1):
            for island, shift in ((100, 0), (window, window // 2), (window, -(window // 2)), (window + 1, 0)):
                reads.append(cases.straddle(rng, length, edge + shift, island, period=1 + len(reads) % 3))
            reads.append(model.repeat(rng, 2, length))  # every window bad: the count is the number of windows
    want = check(ctx, reads)
    assert (want > 0).sum() > len(reads) * 3 // 4
    for T in (10, 300):
        check(ctx, reads[::7], T)


def test_short_runs_of_a_last_span(ctx):
    """windows = 64 r and 64 r + 1 for every run r the rule can give: the last lane's run is full, then one window spills into the
    next size of run; repeat islands across the first and the last lane's edges"""
    window, span = api.complexity_window(), api.complexity_span()
    warm = window - 1
    rng = np.random.default_rng(12)
    reads = []
    for run in range(16, span // 64 + 1, 16):
        for windows in (64 * run - 1, 64 * run, 64 * run + 1):
            if windows > span:
                continue
            length = windows + warm
            reads.append(model.repeat(rng, 3, length))
            for edge in (run, run + warm, 63 * run, 63 * run + warm):
                reads.append(cases.straddle(rng, length, min(edge, length - 1), 100, period=1 + len(reads) % 3))
            reads.append(model.random_seq(rng, span) + model.repeat(rng, 2, length))  # ... as the second span of a read
    want = check(ctx, reads)
    assert (want > 0).all()


def test_crowd_takes_a_second_trip(ctx):
    span = api.complexity_span()
    n_waves = ctx.device_info()["n_cu"] * WAVES_PER_CU
    rng = np.random.default_rng(10)
    big = [model.repeat(rng, 3, 2 * span + 500) + model.random_seq(rng, span), model.random_seq(rng, span + 99) + model.repeat(rng, 1, 3000)]
    n = n_waves * 9 // 4
    lengths = rng.integers(64, 160, size=n)
    lengths[rng.integers(0, n, size=n // 50)] = rng.integers(0, 64, size=n // 50)  # no span: equal neighbours in the segment table
    lengths[:3] = (5, 0, 63)
    lengths[-3:] = (63, 0, 7)
    unit = model.repeat(rng, 2, 200)
    noise = model.random_seq(rng, 4096)
    reads = [big[0]]
    for i, L in enumerate(lengths):
        L = int(L)
        a = int(rng.integers(0, 4096 - 160))
        reads.append(unit[:L] if i % 3 == 0 else noise[a:a + L] if i % 3 == 1 else noise[a:a + L // 2] + unit[:L - L // 2])
    reads.append(big[1])
    spans = sum((model.windows(len(r)) + span - 1) // span for r in reads)
    assert spans > 2 * n_waves + n_waves // 8  # every wave takes two spans, and more than an eighth of them a third
    want = check(ctx, reads)
    assert (want > 0).sum() > len(reads) // 4 and (want == 0).sum() > len(reads) // 4
