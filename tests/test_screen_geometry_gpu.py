"""flx_screen_hits at the LAUNCH GEOMETRY test_screen_gpu.py never reaches, against tests/_screen_model.py (hits_many) for equality,
in the three filter forms.  The batches come from tests/_geometry_cases.py; tests/test_geometry_cases.py proves on a CPU that they
are what is said here.

k_screen_hits (csrc/screen.hip) is persistent: gridDim.x * (kScreenThreads / 64) waves walk the spans with `sp += n_waves`, and the
grid is n_cu workgroups in the LDS form and 2 n_cu in the pre12 and exact forms.  The largest batch of test_screen_gpu.py has under
300 spans, so no wave of any test has come round that loop a second time.

  the crowd           at least 2.5 * (2 n_cu * 16) spans, sized from device_info()["n_cu"]: the first test in which `sp += n_waves`
                      gives a wave a second span (every wave) and a third (half of them; five in the LDS form), that is a second
                      binary search in seg_start, a second prefetch prologue and a second atomicAdd by the same wave.  Reads of
                      kScreenSpan + 15, 2 kScreenSpan + 16 and 40 000 bases at the start, in the middle and at the end of processing
                      order put the spans of ONE read into different rounds of different waves; reads below 16 bases (no span: equal
                      neighbours in seg_start) alone, in runs, and as the first three and the last three reads are the edges of the
                      binary search (lo stays 0 over equal entries; hi = n_reads is never a read)
  2047, 2048, 2049    reads: n_reads + 1 counts through flx_exclusive_scan_u32 are SCAN_TILE, SCAN_TILE + 1, SCAN_TILE + 2 (csrc/sort.hip):
                      one full tile, then a second tile of one and of two entries, the first of which is the sentinel counts[n_reads]
                      alone; k_screen_segments launches (n + 1 + 255) / 256 blocks, for 2048 reads the sentinel has a block of its own

each with order = NULL, the length order, and a random permutation under which the processing order stays the designed one.  Planes
are filled with the contaminant's own sequence between the reads; the host-array form prefills the hits with 0xA5."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import _geometry_cases as geo
import _screen_model as model
from filtlong_amd import api
from test_screen_gpu import make_set, pack

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE_READS = (geo.SCAN_TILE - 1, geo.SCAN_TILE, geo.SCAN_TILE + 1)
ORDERS = ("none", "length", "random")


@pytest.fixture(scope="module")
def ref5k():
    return model.random_seq(np.random.default_rng(101), 5000)


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


class Batch:
    """reads in processing order; the call's arrays and the reads in input order for each of the three orders"""

    def __init__(self, ref, n_reads, seed):
        self.ref = ref
        self.proc, self.places = geo.crowd(ref, n_reads, seed)
        self.spans = int(geo.spans_of(self.proc).sum())
        self._packed = {}

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

    def want(self, x, how):
        return model.hits_many(x, self.packed(how)[0])

    def check(self, ctx, ks, x, how):
        reads, plane, offsets, lengths, order = self.packed(how)
        got = ctx.screen_hits(plane, offsets, lengths, ks, order=order)
        want = model.hits_many(x, reads)
        bad = np.flatnonzero(got != want)
        assert len(bad) == 0, (len(bad), [(int(i), len(reads[i]), int(got[i]), int(want[i])) for i in bad[:10]])
        return got


@pytest.fixture(scope="module")
def crowd(ctx, ref5k):
    n_cu = ctx.device_info()["n_cu"]
    b = Batch(ref5k, geo.crowd_reads(n_cu), 5)
    assert b.spans >= 2.5 * (2 * n_cu * geo.SCREEN_WAVES)  # every wave of the widest grid takes two spans, half of them three
    return b


@pytest.fixture(scope="module")
def tiles(ref5k):
    return {n: Batch(ref5k, n, 6) for n in TILE_READS}


@pytest.fixture(scope="module")
def set5k(ctx, ref5k):
    ks = make_set(ctx, [ref5k])
    yield ks, model.build_set([ref5k])
    ks.close()


@pytest.fixture(scope="module")
def set2m(ctx, ref5k):
    """X of 2 Mbp (the 5 kbp contaminant inside it): no 10-mer table, the 12-mer prefilter alone in front of the bitmap"""
    big = [ref5k + model.random_seq(np.random.default_rng(55), 2000000 - 5000)]
    ks = make_set(ctx, big)
    yield ks, model.build_set(big)
    ks.close()


@pytest.mark.parametrize("how", ORDERS)
def test_crowd_lds_form(ctx, set5k, crowd, how):
    ks, x = set5k
    got = crowd.check(ctx, ks, x, how)
    assert ctx.last_screen_filter() == "lds"
    assert (got > 0).sum() > len(got) // 4 and (got == 0).sum() > len(got) // 4  # hits and misses all through the batch
    if how != "length":  # the long reads' hits were added by many waves in different rounds
        reads = crowd.packed(how)[0]
        long_ones = [i for i, r in enumerate(reads) if len(r) >= geo.SCREEN_SPAN]
        assert len(long_ones) == 9 and all(got[i] > len(reads[i]) // 4 for i in long_ones)


@pytest.mark.parametrize("n_reads", TILE_READS)
def test_scan_tile_edges_lds_form(ctx, set5k, tiles, n_reads):
    ks, x = set5k
    for how in ORDERS:
        tiles[n_reads].check(ctx, ks, x, how)
        assert ctx.last_screen_filter() == "lds"


@pytest.mark.parametrize("how", ORDERS)
def test_crowd_pre12_form(ctx, set2m, crowd, how):
    ks, x = set2m
    assert len(ks) == len(x)
    crowd.check(ctx, ks, x, how)
    assert ctx.last_screen_filter() == "pre12"


@pytest.mark.parametrize("n_reads", TILE_READS)
def test_scan_tile_edges_pre12_form(ctx, set2m, tiles, n_reads):
    ks, x = set2m
    for how in ORDERS:
        tiles[n_reads].check(ctx, ks, x, how)
        assert ctx.last_screen_filter() == "pre12"


def test_exact_form(ref5k, crowd, tiles, tmp_path):
    """FLX_KMER_PREFILTER=0 is read when a set is finalized: one child process builds the set without prefilters and asks the bitmap
    alone, about the crowd and the three batches at the scan's tile edge, each in its three orders"""
    src, dst = str(tmp_path / "in.npz"), str(tmp_path / "out.json")
    calls = [(batch, how) for batch in [crowd] + [tiles[n] for n in TILE_READS] for how in ORDERS]
    arrays = {"ref": np.frombuffer(ref5k, dtype=np.uint8), "more": np.array(len(calls) - 1)}
    for k, (batch, how) in enumerate(calls):
        tag = "" if k == 0 else "_%d" % (k - 1)
        _, plane, offsets, lengths, order = batch.packed(how)
        arrays["plane" + tag], arrays["offsets" + tag], arrays["lengths" + tag] = plane, offsets, lengths
        if order is not None:
            arrays["order" + tag] = order
    np.savez(src, **arrays)
    env = dict(os.environ, FLX_KMER_PREFILTER="0", PYTHONPATH=ROOT)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_screen_worker.py"), src, dst], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=300)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    out = json.load(open(dst))
    assert out["filter"] == "exact" and out["filter_more"] == "exact" and len(out["more"]) == len(calls) - 1
    x = model.build_set([ref5k])
    for (batch, how), got in zip(calls, [out["hits"]] + out["more"]):
        want = batch.want(x, how)
        bad = np.flatnonzero(np.array(got, dtype=np.uint32) != want)
        assert len(bad) == 0, (len(batch.proc), how, len(bad), [(int(i), int(got[i]), int(want[i])) for i in bad[:10]])


def test_one_context_shrinking_and_growing(ctx, set5k, ref5k, crowd):
    """the crowd, a one-read batch, a batch without a hit or a span to spare, the crowd again: counts, seg_start and its sentinel live
    in the context's scratch, and nothing of the larger call may be left in the smaller"""
    ks, x = set5k
    first = crowd.check(ctx, ks, x, "none")
    rng = np.random.default_rng(17)
    for one in (ref5k[300:400], ref5k[:15], b""):
        plane, offsets, lengths = pack([one], ref5k)
        if len(plane) == 0:
            plane = np.frombuffer(ref5k[:16], dtype=np.uint8).copy()  # (a plane of no byte has no address)
        assert ctx.screen_hits(plane, offsets, lengths, ks).tolist() == [model.hits(x, one)]
    quiet = [model.random_seq(rng, int(n)) for n in rng.integers(0, 200, size=300)]
    plane, offsets, lengths = pack(quiet, ref5k)
    got = ctx.screen_hits(plane, offsets, lengths, ks)
    assert (got == model.hits_many(x, quiet)).all() and (got == 0).all()
    assert (crowd.check(ctx, ks, x, "none") == first).all()
