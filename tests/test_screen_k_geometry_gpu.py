"""flx_screenset_hits at the LAUNCH GEOMETRY test_screen_k_gpu.py never reaches, against tests/_screen_k_model.py (hits_many) for
equality.  The batches come from tests/_geometry_cases.py, as in test_screen_geometry_gpu.py.

k_screen_hits_hash (csrc/screen_hash.hip) is persistent: gridDim.x * 4 waves walk the spans with `sp += n_waves`; the grid is what the
device keeps resident, at most 8 waves a SIMD, i.e. at most 32 n_cu waves.

  the crowd          at least 2.5 * (2 n_cu * 16) = 80 n_cu spans: every wave takes a second span and most a third, that is a second
                     binary search in seg_start, a second prefetch prologue and a second atomicAdd by the same wave; long reads at
                     the start, in the middle and at the end of processing order put the spans of ONE read into different rounds of
                     different waves; reads below K bases (no span: equal neighbours in seg_start) alone, in runs, first and last
  fewer              a batch of a few hundred spans: most waves find nothing to do
  one read, no span  a single read; reads that all have zero windows (seg_start is all zero: no wave enters the loop)
  255 .. 257 reads   k_screen_segments launches (n + 1 + 255) / 256 blocks: for 255 reads the sentinel counts[n_reads] is the last
                     thread of the only block, for 256 it has a block of its own

each with order = NULL, the length order, and a random permutation under which the processing order stays the designed one."""
import numpy as np
import pytest

import _geometry_cases as geo
import _screen_k_model as model
from filtlong_amd import api
from test_screen_k_gpu import make_set, pack

pytestmark = pytest.mark.gpu
ORDERS = ("none", "length", "random")
KS = (17, 24, 31)


@pytest.fixture(scope="module")
def ref5k():
    return model.random_seq(np.random.default_rng(101), 5000)


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def sets(ctx, ref5k):
    made = {k: (make_set(ctx, k, [[ref5k]]), model.build_set([ref5k], k)) for k in KS}
    yield made
    for ss, _ in made.values():
        ss.close()


class Batch:
    """reads in processing order; the call's arrays and the reads in input order for each of the three orders"""

    def __init__(self, ref, n_reads, seed):
        self.ref = ref
        self.proc, self.places = geo.crowd(ref, n_reads, seed)
        self._packed = {}

    def spans(self, k):
        return sum((model.windows(len(r), k) + geo.SCREEN_SPAN - 1) // geo.SCREEN_SPAN for r in self.proc)

    def packed(self, how):
        if how not in self._packed:
            n = len(self.proc)
            if how == "random":  # the read processed at place i is still proc[i]; the plane is in another order
                order = np.random.default_rng(n).permutation(n).astype(np.uint32)
                reads = geo.arrange(self.proc, order)
            else:
                reads = self.proc
                order = None
            plane, offsets, lengths = pack(reads, self.ref)
            if how == "length":
                order = api.length_order(lengths)
            self._packed[how] = (reads, plane, offsets, lengths, order)
        return self._packed[how]

    def check(self, ctx, ss, x, k, how):
        reads, plane, offsets, lengths, order = self.packed(how)
        got = ctx.screenset_hits(plane, offsets, lengths, ss, order=order)
        want = model.hits_many(x, reads, k)
        bad = np.flatnonzero(got != want)
        assert len(bad) == 0, (len(bad), [(int(i), len(reads[i]), int(got[i]), int(want[i])) for i in bad[:10]])
        return got


@pytest.fixture(scope="module")
def crowd(ctx, ref5k):
    n_cu = ctx.device_info()["n_cu"]
    b = Batch(ref5k, 2 * geo.crowd_reads(n_cu), 5)  # (twice the bitmap's crowd: at K = 31 half of its short reads have no window)
    assert b.spans(31) >= 2.5 * 32 * n_cu  # every wave of the widest grid the device can hold takes two spans, half of them three
    return b


@pytest.mark.parametrize("how", ORDERS)
@pytest.mark.parametrize("k", KS)
def test_crowd(ctx, sets, crowd, k, how):
    ss, x = sets[k]
    got = crowd.check(ctx, ss, x, k, how)
    assert ctx.last_screen_filter() == "hash"
    assert (got > 0).sum() > len(got) // 8 and (got == 0).sum() > len(got) // 4  # hits and misses all through the batch
    if how != "length":  # the long reads' hits were added by many waves in different rounds
        reads = crowd.packed(how)[0]
        long_ones = [i for i, r in enumerate(reads) if len(r) >= geo.SCREEN_SPAN]
        assert len(long_ones) == 9 and all(got[i] > len(reads[i]) // 8 for i in long_ones)


@pytest.mark.parametrize("n_reads", (255, 256, 257, 300))
def test_fewer_spans_than_waves_and_the_segment_kernel_edges(ctx, sets, ref5k, n_reads):
    b = Batch(ref5k, n_reads, 6)
    for k in KS:
        assert 0 < b.spans(k) < 1000
        for how in ORDERS:
            b.check(ctx, sets[k][0], sets[k][1], k, how)


def test_one_context_shrinking_and_growing(ctx, sets, ref5k, crowd):
    """the crowd, one-read batches, a batch in which no read has a window, the crowd again: counts, seg_start and its sentinel live in
    the context's scratch, and nothing of the larger call may be left in the smaller"""
    k = 24
    ss, x = sets[k]
    first = crowd.check(ctx, ss, x, k, "none")
    rng = np.random.default_rng(17)
    for one in (ref5k[300:400], ref5k[:k], ref5k[:k - 1], b"", ref5k[:geo.SCREEN_SPAN + k]):
        plane, offsets, lengths = pack([one], ref5k)
        if len(plane) == 0:
            plane = np.frombuffer(ref5k[:16], dtype=np.uint8).copy()  # (a plane of no byte has no address)
        assert ctx.screenset_hits(plane, offsets, lengths, ss).tolist() == [model.hits(x, one, k)] == [model.windows(len(one), k)]
    none = [ref5k[a:a + int(n)] for a, n in zip(rng.integers(0, 4000, size=300), rng.integers(0, k, size=300))]
    plane, offsets, lengths = pack(none, ref5k)
    got = ctx.screenset_hits(plane, offsets, lengths, ss)
    assert (got == 0).all() and max(len(r) for r in none) == k - 1
    quiet = [model.random_seq(rng, int(n)) for n in rng.integers(0, 200, size=300)]
    plane, offsets, lengths = pack(quiet, ref5k)
    got = ctx.screenset_hits(plane, offsets, lengths, ss)
    assert (got == model.hits_many(x, quiet, k)).all() and (got == 0).all()
    assert (crowd.check(ctx, ss, x, k, "none") == first).all()
