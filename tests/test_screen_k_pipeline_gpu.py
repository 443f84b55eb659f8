"""flx_pipeline_set_screenset: test_screen_pipeline_gpu.py with a ScreenSet of 24-mers in place of the bitmap.  A pipeline with the
hashed screen gives what the same pipeline gives without it, with the pass flags of the reads the MODEL excludes
(tests/_screen_k_model.py) and of all their children cleared afterwards — in Phred mode (two planes a chunk) and in k-mer mode (one),
with many small chunks and with slots that grow, with --split_window_q children and --trim --split children of an excluded parent.
A pipeline takes one of set_screen and set_screenset; without either nothing of the screen is launched."""
import ctypes as C

import numpy as np
import pytest

import _qsplit_model as qmodel
import _screen_k_model as model
from filtlong_amd import api
from test_screen_pipeline_gpu import SAME, chunked, expect

pytestmark = pytest.mark.gpu
PERCENT = 10.0
K = 24


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def world(ctx):
    """a contaminant X of 5 kbp with its set of 24-mers, a genome G of 40 kbp with its 16-mer set, and reads: from G, from X on either
    strand with 5 % substitutions, unrelated, chimeras of both, reads below K bases; qualities with junk stretches"""
    rng = np.random.default_rng(78)
    xref, gref = model.random_seq(rng, 5000), model.random_seq(rng, 40000)
    seqs = []
    for i in range(90):
        kind = i % 6
        n = int(rng.integers(300, 5000))
        if kind in (0, 1):
            s = model.draw(rng, gref, n, 0.03)
        elif kind == 2:
            s = model.draw(rng, xref, min(n, 4000), 0.05)
        elif kind == 3:
            s = model.random_seq(rng, n)
        elif kind == 4:  # G, X, G: --split leaves children of a read the screen excludes
            s = model.draw(rng, gref, 1500, 0.0, 0) + model.draw(rng, xref, 900, 0.01) + model.draw(rng, gref, 1500, 0.0, 0)
        else:            # mostly G with a little X: below 10 %
            s = model.draw(rng, gref, 3000, 0.02) + model.draw(rng, xref, 150, 0.0)
        seqs.append(s)
    seqs += [b"ACGT", b"", xref[:K - 1], xref[:K], xref[100:100 + 2 * K - 1]]
    quals = []
    for s in seqs:
        n = len(s)
        st = [(n // 3, n // 3 + 400)] if n > 1500 and rng.integers(0, 2) else []
        quals.append(qmodel.junk_read(rng, n, st))
    contaminant = [xref[:2000] + b"NNNNNNNNNN" + xref[2000:]]
    xs = api.ScreenSet(ctx, K, 4)
    xs.add_fasta(contaminant)
    xs.finalize()
    gs = api.Kmers(ctx)
    gs.add_assembly_fasta([gref])
    gs.finalize()
    x = model.build_set(contaminant, K)
    assert len(xs) == len(x)
    hits = model.hits_many(x, seqs, K)
    excl = np.array([model.excluded(h, len(s), PERCENT, K) for h, s in zip(hits, seqs)], dtype=np.uint8)
    assert 10 < excl.sum() < len(seqs) - 30
    yield {"seqs": seqs, "quals": quals, "xs": xs, "gs": gs, "hits": hits, "excl": excl, "contaminant": contaminant}
    xs.close()
    gs.close()


def compare(got, base, w):
    want = expect(base, w["excl"])
    assert (got["hits"] == w["hits"]).all(), np.flatnonzero(got["hits"] != w["hits"])[:10]
    assert (got["excluded"] == w["excl"]).all()
    for k in SAME:
        assert got[k].tobytes() == want[k].tobytes(), k
    assert (got["passed"] == want["passed"]).all() and (got["child_passed"] == want["child_passed"]).all()
    return want


@pytest.mark.parametrize("size,grow", [(7, False), (40, True)])
def test_phred_mode(ctx, world, size, grow):
    w = world
    params = api.make_params(min_length=500, min_mean_q=70)
    kw = dict(chunk_bytes=4096 if grow else 1 << 16, chunk_reads=4 if grow else 64, grow=grow)
    base = ctx.score_stream(chunked(w["quals"], size), params, **kw)
    got = ctx.score_stream(list(zip(chunked(w["quals"], size), chunked(w["seqs"], size))), params, exclude=w["xs"], exclude_percent=PERCENT, **kw)
    want = compare(got, base, w)
    assert base["passed"].sum() > want["passed"].sum() > 10  # the screen took reads that had passed, and left others


def test_phred_mode_split_window_q(ctx, world):
    w = world
    params = api.make_params(min_length=200)
    base = ctx.score_stream(chunked(w["quals"], 9), params, chunk_bytes=1 << 16, chunk_reads=16, split_window_q=85)
    got = ctx.score_stream(list(zip(chunked(w["quals"], 9), chunked(w["seqs"], 9))), params, chunk_bytes=1 << 16, chunk_reads=16,
                           split_window_q=85, exclude=w["xs"], exclude_percent=PERCENT)
    want = compare(got, base, w)
    per = np.diff(base["child_offsets"].astype(np.int64))
    assert ((per >= 2) & (w["excl"] != 0)).sum() >= 2, "an excluded parent with children"
    assert base["child_passed"].sum() > want["child_passed"].sum() > 0


@pytest.mark.parametrize("size,grow", [(11, False), (50, True)])
def test_kmer_mode_trim_split(ctx, world, size, grow):
    w = world
    params = api.make_params(min_length=100, trim=True, split=100)
    kw = dict(kmers=w["gs"], chunk_bytes=4096 if grow else 1 << 16, chunk_reads=4 if grow else 64, grow=grow)
    base = ctx.score_stream(chunked(w["seqs"], size), params, **kw)
    got = ctx.score_stream(chunked(w["seqs"], size), params, exclude=w["xs"], exclude_percent=PERCENT, **kw)
    want = compare(got, base, w)
    per = np.diff(base["child_offsets"].astype(np.int64))
    assert ((per >= 2) & (w["excl"] != 0)).sum() >= 5, "the G-X-G chimeras: children of an excluded parent"
    assert base["child_passed"].sum() > want["child_passed"].sum() > 0


def test_exclude_percent_moves_the_decision(ctx, world):
    w = world
    params = api.make_params(min_length=1)
    got = ctx.score_stream([(w["quals"], w["seqs"])], params, chunk_bytes=1 << 20, chunk_reads=256, exclude=w["xs"], exclude_percent=60.0)
    excl60 = np.array([model.excluded(h, len(s), 60.0, K) for h, s in zip(w["hits"], w["seqs"])], dtype=np.uint8)
    assert (got["excluded"] == excl60).all() and (got["hits"] == w["hits"]).all()
    assert 0 < excl60.sum() < w["excl"].sum()
    assert (got["passed"] == ((excl60 == 0) & (np.array([len(s) for s in w["seqs"]]) >= 1))).all()
    # the windows of the decision are L - K + 1: a read of K bases from X is one window and one hit, one of K - 1 bases none
    at = len(w["seqs"]) - 5
    assert list(got["excluded"][at:]) == [0, 0, 0, 1, 1] and list(got["hits"][at:]) == [0, 0, 0, 1, K]


def test_call_order_and_arguments(ctx, world):
    L, w = ctx.L, world
    params = api.make_params()
    pipe = C.c_void_p()
    ctx._check(L.flx_pipeline_create(ctx.h, None, C.byref(params), 1 << 16, 64, C.byref(pipe)))
    try:
        assert L.flx_pipeline_set_screenset(pipe, w["xs"].h, 0.0) == 1 and L.flx_pipeline_set_screenset(pipe, w["xs"].h, 100.5) == 1
        assert L.flx_pipeline_set_screenset(pipe, None, 10.0) == 1
        empty = api.ScreenSet(ctx, K)
        empty.add_fasta([b"ACGTNACGT"])
        assert L.flx_pipeline_set_screenset(pipe, empty.h, 10.0) == 4  # not finalized
        empty.finalize()
        assert L.flx_pipeline_set_screenset(pipe, empty.h, 10.0) == 4  # empty
        empty.close()
        buf, cb, cr = C.c_void_p(), C.c_uint64(), C.c_uint64()
        ctx._check(L.flx_pipeline_next_buffer(pipe, C.byref(buf), C.byref(cb), C.byref(cr)))
        plane, offsets, lengths = api.pack_reads([w["quals"][0]])
        C.memmove(buf, plane.ctypes.data, plane.nbytes)
        ctx._check(L.flx_pipeline_submit(pipe, plane.nbytes, offsets.ctypes.data, lengths.ctypes.data, 1))
        assert L.flx_pipeline_set_screenset(pipe, w["xs"].h, 10.0) == 4  # FLX_ERR_STATE: after a submit
        s, n = api.Scores(), C.c_uint64()
        ctx._check(L.flx_pipeline_finish(pipe, C.byref(s), C.byref(n)))
        assert n.value == 1
        hp, ep = C.c_void_p(), C.c_void_p()
        assert L.flx_pipeline_screen(pipe, C.byref(hp), C.byref(ep)) == 4  # no screen on this pipeline
    finally:
        L.flx_pipeline_destroy(pipe)


def test_one_of_the_two_screens(ctx, world):
    L, w = ctx.L, world
    params = api.make_params()
    bitmap = api.Kmers(ctx)
    bitmap.add_screen_fasta(w["contaminant"])
    bitmap.finalize()
    try:
        calls = [(L.flx_pipeline_set_screen, bitmap.h), (L.flx_pipeline_set_screenset, w["xs"].h)]
        for (first, first_set), (second, second_set) in (calls, calls[::-1]):
            pipe = C.c_void_p()
            ctx._check(L.flx_pipeline_create(ctx.h, None, C.byref(params), 1 << 16, 64, C.byref(pipe)))
            try:
                assert first(pipe, first_set, 10.0) == 0
                assert second(pipe, second_set, 10.0) == 4  # FLX_ERR_STATE
                assert first(pipe, first_set, 20.0) == 0    # the same call again is what it was before: the later percent holds
            finally:
                L.flx_pipeline_destroy(pipe)
    finally:
        bitmap.close()


def test_without_either_call_nothing_of_the_screen_runs(ctx, world):
    """the launches of a pipeline without the flag: none carries the screen's names; with the hashed screen two more a chunk"""
    w = world
    params = api.make_params(min_length=500)
    ctx.timing_enable(True)
    try:
        ctx.timing_reset()
        base = ctx.score_stream(chunked(w["quals"], 16), params, chunk_bytes=1 << 16, chunk_reads=64)
        _, all_launches = ctx.timing_get("")
        assert ctx.timing_get("flx_screen")[1] == 0 and all_launches > 0
        ctx.timing_reset()
        got = ctx.score_stream(list(zip(chunked(w["quals"], 16), chunked(w["seqs"], 16))), params, chunk_bytes=1 << 16, chunk_reads=64,
                               exclude=w["xs"], exclude_percent=PERCENT)
        chunks = len(chunked(w["quals"], 16))
        assert ctx.timing_get("flx_screen")[1] == 2 * chunks  # "flx_screen" and "flx_screen_apply", once a chunk
        assert ctx.timing_get("")[1] == all_launches + 2 * chunks  # and nothing else moved
        assert ctx.last_screen_filter() == "hash"
    finally:
        ctx.timing_enable(False)
    compare(got, base, w)
