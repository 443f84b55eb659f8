"""score_reads(trim_ends_q=) and score_stream(trim_ends_q=) against tests/_endtrim_model.py plus score_reads on the child substrings:
first / last and the child ranges are the model's, a parent's mean_q / window_q are those of the plain call, a child's mean_q /
window_q / passed are the BITS the plain call gives its quality substring as a read of its own, and a read of which the cuts leave
nothing fails.  The pipeline gives, chunk size whatever, what one call gives, and its "endtrim_cuts" are the model's; with the
low-complexity filter as well (a second plane, the sequences) a dropped parent's child fails.  The FLX_ERR_CAPACITY round trip and the FLX_ERR_STATE
refusals of the setters."""
import ctypes as C

import numpy as np
import pytest

import _endtrim_cases as cases
import _endtrim_model as model
from filtlong_amd import _lib, api

pytestmark = pytest.mark.gpu
Q = 90.0
SAME = ("mean_q", "window_q", "passed", "first", "last", "child_offsets", "child_ranges", "child_mean_q", "child_window_q", "child_passed")


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def world(ctx):
    """reads of 0 to 6000 bases and one of more than a span: trimmed at one end or both, untouched, wholly junk, empty"""
    rng = np.random.default_rng(31)
    span = api.endtrim_span()
    quals = cases.mixed_batch(rng, 90, 6000) + [cases.ont_like(rng, span + 2000, 700, 1300), cases.ont_like(rng, 800, 0, 0), b"!" * 30, b"I" * 30,
                                                  cases.ont_like(rng, 320, 30, 30)]  # (the last: long enough for --min_length, its child is not)
    t = api.qsplit_threshold(Q)
    assert t == cases.T90
    cuts = model.batch_cuts(quals, t)
    params = api.make_params(window_size=100, min_length=300, min_mean_q=5.0)
    plane, offsets, lengths = api.pack_reads(quals)
    one = ctx.score_reads(plane, offsets, lengths, params, trim_ends_q=Q, order=api.length_order(lengths))
    plain = ctx.score_reads(plane, offsets, lengths, params)
    return {"quals": quals, "t": t, "cuts": cuts, "params": params, "one": one, "plain": plain}


def chunked(items, size):
    return [items[i:i + size] for i in range(0, len(items), size)]


def test_one_call_against_the_model(ctx, world):
    w = world
    one, quals = w["one"], w["quals"]
    kids, first, last, counts = [], [], [], []
    for q, (h, c) in zip(quals, w["cuts"]):
        n, f, e = model.child_of(int(h), int(c), len(q))
        counts.append(n)
        first.append(f)
        last.append(e)
        if n:
            kids.append((f, e, q[f:e]))
    assert (one["first"] == np.array(first, dtype=np.int32)).all() and (one["last"] == np.array(last, dtype=np.int32)).all()
    assert (one["child_offsets"] == np.concatenate(([0], np.cumsum(counts))).astype(np.uint64)).all()
    assert (one["child_ranges"] == np.array([(f, e) for f, e, _ in kids], dtype=np.int32).reshape(-1, 2)).all()
    # the parents: scored as ever; a read of which nothing is left fails
    assert one["mean_q"].tobytes() == w["plain"]["mean_q"].tobytes() and one["window_q"].tobytes() == w["plain"]["window_q"].tobytes()
    gone = (np.array(first) == -1) & (np.array([len(q) for q in quals]) > 0)
    want_passed = w["plain"]["passed"].copy()
    want_passed[gone] = 0
    assert (one["passed"] == want_passed).all() and gone.sum() >= 5
    # the children: each the bits of a read of its own, its own hard cut-offs included
    plane, offsets, lengths = api.pack_reads([k[2] for k in kids])
    alone = ctx.score_reads(plane, offsets, lengths, w["params"])
    for k, a in (("child_mean_q", "mean_q"), ("child_window_q", "window_q"), ("child_passed", "passed")):
        assert one[k].tobytes() == alone[a].tobytes(), k
    assert len(kids) > 50 and 0 < one["child_passed"].sum() < len(kids) and sum(1 for c in counts if c == 0) > 15
    # (a child that a parent's length lets pass and its own does not)
    assert any(w["plain"]["passed"][i] and not one["child_passed"][int(one["child_offsets"][i])] for i in range(len(quals)) if counts[i])


@pytest.mark.parametrize("size,grow", [(5, False), (30, True)])
def test_the_pipeline_gives_what_one_call_gives(ctx, world, size, grow):
    w = world
    kw = dict(chunk_bytes=4096 if grow else 1 << 17, chunk_reads=4 if grow else 64, grow=grow)
    got = ctx.score_stream(chunked(w["quals"], size), w["params"], trim_ends_q=Q, **kw)
    assert (got["endtrim_cuts"] == w["cuts"]).all(), np.flatnonzero((got["endtrim_cuts"] != w["cuts"]).any(axis=1))[:10]
    for k in SAME:
        assert got[k].tobytes() == w["one"][k].tobytes(), k


def test_with_the_low_complexity_filter(ctx, world):
    """the filter looks at the whole parent (a second plane, the sequences), and a dropped parent's child fails"""
    w = world
    rng = np.random.default_rng(32)
    seqs = [(b"A" * len(q)) if i % 5 == 0 else bytes(rng.choice(list(b"ACGT"), size=len(q)).astype(np.uint8)) for i, q in enumerate(w["quals"])]
    pairs = list(zip(chunked(w["quals"], 9), chunked(seqs, 9)))
    got = ctx.score_stream(pairs, w["params"], chunk_bytes=1 << 17, chunk_reads=16, trim_ends_q=Q, max_low_complexity=50.0)
    assert (got["endtrim_cuts"] == w["cuts"]).all()
    flagged = got["low_complexity"] != 0
    assert flagged.sum() >= 10 and all(not f or i % 5 == 0 for i, f in enumerate(flagged))
    want = {k: v.copy() for k, v in w["one"].items()}
    want["passed"][flagged] = 0
    with_child = 0
    for i in np.flatnonzero(flagged):
        a, b = int(want["child_offsets"][i]), int(want["child_offsets"][i + 1])
        with_child += int(want["child_passed"][a:b].sum())
        want["child_passed"][a:b] = 0
    assert with_child >= 3, "children that had passed, of parents the filter drops"
    for k in SAME:
        assert got[k].tobytes() == want[k].tobytes(), k


def test_capacity_round_trip(ctx, world):
    w = world
    plane, offsets, lengths = api.pack_reads(w["quals"])
    n, nc = len(w["quals"]), len(w["one"]["child_mean_q"])
    out = {"mean_q": np.zeros(n), "window_q": np.zeros(n), "passed": np.zeros(n, np.uint8), "coff": np.zeros(n + 1, np.uint64)}
    cap = 3
    cr, cm, cw, cp = np.zeros(2 * cap, np.int32), np.zeros(cap), np.zeros(cap), np.zeros(cap, np.uint8)
    s = _lib.Scores()
    s.mean_q, s.window_q, s.passed = out["mean_q"].ctypes.data, out["window_q"].ctypes.data, out["passed"].ctypes.data
    s.child_offsets = out["coff"].ctypes.data
    s.child_ranges, s.child_mean_q, s.child_window_q, s.child_passed = cr.ctypes.data, cm.ctypes.data, cw.ctypes.data, cp.ctypes.data
    s.child_capacity = cap
    rc = ctx.L.flx_score_batch_endtrim(ctx.h, plane.ctypes.data, plane.nbytes, offsets.ctypes.data, lengths.ctypes.data, None, n,
                                       C.byref(w["params"]), w["t"], C.byref(s))
    assert rc == 5 and int(s.n_children) == nc > cap  # FLX_ERR_CAPACITY, with the capacity needed
    again = ctx.score_reads(plane, offsets, lengths, w["params"], trim_ends_q=Q, child_capacity=2)  # (retries with the reported size)
    for k in SAME:
        assert again[k].tobytes() == w["one"][k].tobytes(), k
    # the argument checks of flx_score_batch_adapters
    s.child_offsets = None
    assert ctx.L.flx_score_batch_endtrim(ctx.h, plane.ctypes.data, plane.nbytes, offsets.ctypes.data, lengths.ctypes.data, None, n,
                                         C.byref(w["params"]), w["t"], C.byref(s)) == 1
    s.child_offsets = out["coff"].ctypes.data
    trim = api.make_params(trim=True)
    assert ctx.L.flx_score_batch_endtrim(ctx.h, plane.ctypes.data, plane.nbytes, offsets.ctypes.data, lengths.ctypes.data, None, n,
                                         C.byref(trim), w["t"], C.byref(s)) == 1
    assert ctx.L.flx_score_batch_endtrim(ctx.h, plane.ctypes.data, plane.nbytes, offsets.ctypes.data, lengths.ctypes.data, None, n,
                                         C.byref(w["params"]), 2**32, C.byref(s)) == 1


def test_setters_and_their_refusals(ctx, world):
    L = ctx.L
    params = api.make_params()
    pipe = C.c_void_p()
    ad = api.Adapters([b"AATGTACTTCGTTCAGTTACGTATTGCT"], errors=20, window=80)
    ctx._check(L.flx_pipeline_create(ctx.h, None, C.byref(params), 1 << 16, 64, C.byref(pipe)))
    try:
        cp = C.c_void_p()
        assert L.flx_pipeline_endtrim(pipe, C.byref(cp)) == 4  # not set on this pipeline
        assert L.flx_pipeline_set_endtrim(pipe, 0.0) == 1 and L.flx_pipeline_set_endtrim(pipe, 100.0) == 1
        ctx._check(L.flx_pipeline_set_endtrim(pipe, Q))
        assert L.flx_pipeline_set_qsplit(pipe, 85.0) == 4  # FLX_ERR_STATE: not together with split_window_q
        assert b"do not compose" in L.flx_last_error(ctx.h)
        assert L.flx_pipeline_set_adapters(pipe, ad.h) == 4  # ... nor with adapters
        assert b"do not compose" in L.flx_last_error(ctx.h)
        buf, cb, cr = C.c_void_p(), C.c_uint64(), C.c_uint64()
        ctx._check(L.flx_pipeline_next_buffer(pipe, C.byref(buf), C.byref(cb), C.byref(cr)))
        lengths = np.array([16], dtype=np.int32)
        offsets = np.zeros(1, dtype=np.uint64)
        C.memmove(buf, b"!" + b"I" * 15, 16)  # (one junk base in front of fifteen good ones: the head cut is 1, the tail cut 0)
        ctx._check(L.flx_pipeline_submit(pipe, 16, offsets.ctypes.data, lengths.ctypes.data, 1))
        assert L.flx_pipeline_set_endtrim(pipe, Q) == 4  # FLX_ERR_STATE: after submit
        s, n_all = _lib.Scores(), C.c_uint64()
        ctx._check(L.flx_pipeline_finish(pipe, C.byref(s), C.byref(n_all)))
        ctx._check(L.flx_pipeline_endtrim(pipe, C.byref(cp)))
        got = np.ctypeslib.as_array(C.cast(cp, C.POINTER(C.c_uint32)), shape=(2,)).copy()
        assert n_all.value == 1 and tuple(got) == (1, 0)
    finally:
        L.flx_pipeline_destroy(pipe)
    for first in ("qsplit", "adapters"):  # ... in either order
        ctx._check(L.flx_pipeline_create(ctx.h, None, C.byref(params), 1 << 16, 64, C.byref(pipe)))
        try:
            ctx._check(L.flx_pipeline_set_qsplit(pipe, 85.0) if first == "qsplit" else L.flx_pipeline_set_adapters(pipe, ad.h))
            assert L.flx_pipeline_set_endtrim(pipe, Q) == 4
            assert b"do not compose" in L.flx_last_error(ctx.h)
        finally:
            L.flx_pipeline_destroy(pipe)
    trim = api.make_params(trim=True)
    ctx._check(L.flx_pipeline_create(ctx.h, None, C.byref(trim), 1 << 16, 64, C.byref(pipe)))
    try:
        assert L.flx_pipeline_set_endtrim(pipe, Q) == 1
    finally:
        L.flx_pipeline_destroy(pipe)
    ad.close()


def test_without_the_setter_the_plain_pipeline(ctx, world):
    """the launches of a pipeline without the flag: none carries the feature's name, and the results are those of one flx_score_batch"""
    w = world
    ctx.timing_enable(True)
    try:
        ctx.timing_reset()
        base = ctx.score_stream(chunked(w["quals"], 16), w["params"], chunk_bytes=1 << 17, chunk_reads=64)
        assert ctx.timing_get("flx_endtrim")[1] == 0 and ctx.timing_get("")[1] > 0
        ctx.timing_reset()
        ctx.score_stream(chunked(w["quals"], 16), w["params"], chunk_bytes=1 << 17, chunk_reads=64, trim_ends_q=Q)
        assert ctx.timing_get("flx_endtrim")[1] == len(chunked(w["quals"], 16))  # once a chunk
    finally:
        ctx.timing_enable(False)
    for k in ("mean_q", "window_q", "passed"):
        assert base[k].tobytes() == w["plain"][k].tobytes(), k
    assert "endtrim_cuts" not in base and base["child_offsets"].max() == 0
