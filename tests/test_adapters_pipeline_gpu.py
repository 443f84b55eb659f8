"""flx_pipeline_set_adapters: a Phred-mode pipeline with adapters gives, chunk size whatever, what ONE flx_score_batch_adapters call
gives for all reads, and keys equal to the model's (tests/_adapters_model.py); with a screen as well, the reads the screen's MODEL
excludes fail together with their child.  Call-order errors; without set_adapters the pipeline is the plain one."""
import ctypes as C

import numpy as np
import pytest

import _adapters_cases as cases
import _adapters_model as model
import _screen_model as smodel
from filtlong_amd import api, synth

pytestmark = pytest.mark.gpu
WINDOW, ERRORS, PERCENT = 80, 20, 10.0
SAME = ("mean_q", "window_q", "passed", "first", "last", "child_offsets", "child_ranges", "child_mean_q", "child_window_q", "child_passed")


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def world(ctx):
    """reads of 0 to 4000 bases: two in three carry an adapter at one end or both; a contaminant X, and reads from X with adapters"""
    rng = np.random.default_rng(99)
    seqs = [cases.LIGATION, cases.random_adapter(rng, 20)]
    xref = smodel.random_seq(rng, 4000)
    reads = []
    for i in range(72):
        n = int(rng.integers(100, 4000))
        body = smodel.draw(rng, xref, min(n, 3000), 0.03) if i % 4 == 0 else cases.random_seq(rng, n)
        head = cases.random_seq(rng, int(rng.integers(0, 15))) + cases.substitute(rng, seqs[i % 2], 2) if i % 3 != 2 else b""
        tail = model.revcomp(seqs[(i // 2) % 2]) + cases.random_seq(rng, int(rng.integers(0, 10))) if i % 3 != 1 else b""
        reads.append(head + body + tail)
    reads += [b"", b"ACGT", cases.LIGATION, cases.LIGATION + model.revcomp(cases.LIGATION), cases.random_seq(rng, 79), cases.random_seq(rng, 1030)]
    quals = [synth.qual_read(900 + i, len(r)).tobytes() if len(r) else b"" for i, r in enumerate(reads)]
    keys = model.keys_of(reads, WINDOW, model.patterns(seqs), ERRORS)
    xs = api.Kmers(ctx)
    xs.add_screen_fasta([xref])
    xs.finalize()
    x = smodel.build_set([xref])
    hits = np.array([smodel.hits(x, s) for s in reads], dtype=np.uint32)
    excl = np.array([smodel.excluded(h, len(s), PERCENT) for h, s in zip(hits, reads)], dtype=np.uint8)
    ad = api.Adapters(seqs, errors=ERRORS, window=WINDOW)
    params = api.make_params(window_size=100, min_length=300, min_mean_q=5.0)
    splane, offsets, lengths = cases.pack(reads)
    qplane, _, _ = cases.pack(quals)
    one = ctx.score_reads(qplane, offsets, lengths, params, adapters=ad, seq_plane=splane)
    yield {"reads": reads, "quals": quals, "keys": keys, "xs": xs, "hits": hits, "excl": excl, "ad": ad, "params": params, "one": one}
    xs.close()
    ad.close()


def chunked(items, size):
    return [items[i:i + size] for i in range(0, len(items), size)]


def pairs(w, size):
    return list(zip(chunked(w["quals"], size), chunked(w["reads"], size)))


@pytest.mark.parametrize("size,grow", [(5, False), (30, True)])
def test_adapters_alone(ctx, world, size, grow):
    w = world
    kw = dict(chunk_bytes=4096 if grow else 1 << 16, chunk_reads=4 if grow else 64, grow=grow)
    got = ctx.score_stream(pairs(w, size), w["params"], adapters=w["ad"], **kw)
    assert (got["adapter_keys"] == w["keys"]).all(), np.flatnonzero((got["adapter_keys"] != w["keys"]).any(axis=1))[:10]
    for k in SAME:
        assert got[k].tobytes() == w["one"][k].tobytes(), k
    per = np.diff(got["child_offsets"].astype(np.int64))
    assert per.max() == 1 and per.sum() > 40 and (got["first"] == -1).sum() >= 2 and 0 < got["child_passed"].sum() < per.sum()


def test_adapters_with_a_screen(ctx, world):
    """one sequence plane serves both; the screen looks at the whole parent, and an excluded parent's child fails"""
    w = world
    got = ctx.score_stream(pairs(w, 9), w["params"], chunk_bytes=1 << 16, chunk_reads=16, adapters=w["ad"], exclude=w["xs"], exclude_percent=PERCENT)
    assert (got["adapter_keys"] == w["keys"]).all() and (got["hits"] == w["hits"]).all() and (got["excluded"] == w["excl"]).all()
    want = {k: v.copy() for k, v in w["one"].items()}
    want["passed"][w["excl"] != 0] = 0
    with_child = 0
    for i in np.flatnonzero(w["excl"]):
        a, b = int(want["child_offsets"][i]), int(want["child_offsets"][i + 1])
        with_child += int(want["child_passed"][a:b].sum())
        want["child_passed"][a:b] = 0
    assert with_child >= 5, "children that had passed, of parents the screen excludes"
    for k in SAME:
        assert got[k].tobytes() == want[k].tobytes(), k


def test_call_order_and_arguments(ctx, world):
    L, w = ctx.L, world
    params = api.make_params()
    pipe = C.c_void_p()
    ctx._check(L.flx_pipeline_create(ctx.h, None, C.byref(params), 1 << 16, 64, C.byref(pipe)))
    try:
        kp = C.c_void_p()
        assert L.flx_pipeline_adapters(pipe, C.byref(kp)) == 4  # no adapters on this pipeline
        assert L.flx_pipeline_set_adapters(pipe, None) == 1
        ctx._check(L.flx_pipeline_set_adapters(pipe, w["ad"].h))
        assert L.flx_pipeline_set_qsplit(pipe, 85.0) == 4      # not together with split_window_q
        ctx._check(L.flx_pipeline_set_screen(pipe, w["xs"].h, 10.0))
        buf, cb, cr = C.c_void_p(), C.c_uint64(), C.c_uint64()
        ctx._check(L.flx_pipeline_next_buffer(pipe, C.byref(buf), C.byref(cb), C.byref(cr)))
        assert L.flx_pipeline_set_adapters(pipe, w["ad"].h) == 4  # FLX_ERR_STATE: after the first next_buffer
    finally:
        L.flx_pipeline_destroy(pipe)
    ctx._check(L.flx_pipeline_create(ctx.h, None, C.byref(params), 1 << 16, 64, C.byref(pipe)))
    try:
        ctx._check(L.flx_pipeline_set_qsplit(pipe, 85.0))
        assert L.flx_pipeline_set_adapters(pipe, w["ad"].h) == 4  # ... in either order
    finally:
        L.flx_pipeline_destroy(pipe)
    ctx._check(L.flx_pipeline_create(ctx.h, w["xs"].h, C.byref(params), 1 << 16, 64, C.byref(pipe)))
    try:
        assert L.flx_pipeline_set_adapters(pipe, w["ad"].h) == 4  # a pipeline with a non-empty set is in k-mer mode
    finally:
        L.flx_pipeline_destroy(pipe)
    trim = api.make_params(trim=True)
    ctx._check(L.flx_pipeline_create(ctx.h, None, C.byref(trim), 1 << 16, 64, C.byref(pipe)))
    try:
        assert L.flx_pipeline_set_adapters(pipe, w["ad"].h) == 1
    finally:
        L.flx_pipeline_destroy(pipe)


def test_without_set_adapters_the_plain_pipeline(ctx, world):
    """the launches of a pipeline without the flag: none carries the adapters' name, and the results are those of one flx_score_batch"""
    w = world
    ctx.timing_enable(True)
    try:
        ctx.timing_reset()
        base = ctx.score_stream(chunked(w["quals"], 16), w["params"], chunk_bytes=1 << 16, chunk_reads=64)
        assert ctx.timing_get("flx_adapters")[1] == 0 and ctx.timing_get("")[1] > 0
        ctx.timing_reset()
        ctx.score_stream(pairs(w, 16), w["params"], chunk_bytes=1 << 16, chunk_reads=64, adapters=w["ad"])
        assert ctx.timing_get("flx_adapters")[1] == len(chunked(w["quals"], 16))  # once a chunk
    finally:
        ctx.timing_enable(False)
    plane, offsets, lengths = api.pack_reads(w["quals"])
    one = ctx.score_reads(plane, offsets, lengths, w["params"])
    for k in ("mean_q", "window_q", "passed"):
        assert base[k].tobytes() == one[k].tobytes(), k
    assert (base["first"] == -1).all() and base["child_offsets"].max() == 0
