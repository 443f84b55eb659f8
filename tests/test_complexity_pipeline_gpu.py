"""flx_pipeline_set_complexity: a pipeline with the low-complexity filter gives what the same pipeline gives without it, with the pass
flags of the reads the MODEL flags (tests/_complexity_model.py) and of all their children cleared afterwards, and every score bit for
bit what it was — in Phred mode (two planes a chunk) alone, with a screen, with adapters and with both, with --split_window_q
children, and in k-mer mode (one plane) with --trim --split children of a flagged parent.  Chunks of one to a few reads put a flagged
read first, last and alone in a chunk.  Without set_complexity nothing of the filter is launched."""
import ctypes as C

import numpy as np
import pytest

import _adapters_cases as acases
import _complexity_model as model
import _qsplit_model as qmodel
import _screen_model as smodel
from filtlong_amd import api

pytestmark = pytest.mark.gpu
PERCENT, SCORE = 50.0, 20
SAME = ("mean_q", "window_q", "first", "last", "child_offsets", "child_ranges", "child_mean_q", "child_window_q")


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def world(ctx):
    """a genome G of 40 kbp with its set, a contaminant X of 4 kbp with its screen set, adapters, and reads: from G, repeat junk,
    chimeras G + junk + G above and below 50 %, reads from X, reads below 64 bases; qualities with junk stretches"""
    rng = np.random.default_rng(4242)
    gref, xref = smodel.random_seq(rng, 40000), smodel.random_seq(rng, 4000)
    adapter_seqs = [acases.LIGATION, acases.random_adapter(rng, 20)]
    seqs = []
    for i in range(66):
        kind = i % 6
        n = int(rng.integers(300, 4000))
        if kind in (0, 1):
            s = smodel.draw(rng, gref, n, 0.03)
        elif kind == 2:
            s = model.repeat(rng, 1 + i // 6 % 6, n, rate=0.05)
        elif kind == 3:  # G, junk, G: --split leaves children of a read the filter flags (junk is 60 % of it)
            s = smodel.draw(rng, gref, 600, 0.0, 0) + model.repeat(rng, 2 + i % 3, 1800) + smodel.draw(rng, gref, 600, 0.0, 0)
        elif kind == 4:  # mostly G with a repeat island: below 50 %
            s = smodel.draw(rng, gref, 2500, 0.02) + model.repeat(rng, 3, 600)
        else:
            s = acases.LIGATION + smodel.draw(rng, xref, min(n, 3000), 0.03) if i % 12 == 5 else acases.LIGATION + model.repeat(rng, 2, n)
        seqs.append(s)
    seqs += [b"ACGT", b"", b"A" * 63, b"A" * 64, model.repeat(rng, 3, 100)]
    quals = []
    for s in seqs:
        n = len(s)
        st = [(n // 3, n // 3 + 400)] if n > 1500 and rng.integers(0, 2) else []
        quals.append(qmodel.junk_read(rng, n, st))
    gs = api.Kmers(ctx)
    gs.add_assembly_fasta([gref])
    gs.finalize()
    xs = api.Kmers(ctx)
    xs.add_screen_fasta([xref])
    xs.finalize()
    ad = api.Adapters(adapter_seqs, errors=20, window=80)
    bad = model.bad_many(seqs, SCORE)
    low = model.flagged_many(bad, [len(s) for s in seqs], PERCENT)
    assert 15 < low.sum() < len(seqs) - 30 and low[3] and not low[4] and low[-2] and not low[-3]
    yield {"seqs": seqs, "quals": quals, "gs": gs, "xs": xs, "ad": ad, "bad": bad, "low": low}
    gs.close()
    xs.close()
    ad.close()


def chunks_of(items, sizes):
    """consecutive chunks whose sizes cycle through `sizes`"""
    out, at, k = [], 0, 0
    while at < len(items):
        out.append(items[at:at + sizes[k % len(sizes)]])
        at += sizes[k % len(sizes)]
        k += 1
    return out


SIZES = (1, 3, 2, 1, 4)  # (11 a cycle, the kinds of reads 6: every kind comes to every place of a chunk)


def placements(low, sizes=SIZES):
    """how many flagged reads are the first of a chunk of several, the last of one, and alone in a chunk"""
    first = last = alone = 0
    for c in chunks_of(list(range(len(low))), sizes):
        first += len(c) > 1 and bool(low[c[0]])
        last += len(c) > 1 and bool(low[c[-1]])
        alone += len(c) == 1 and bool(low[c[0]])
    return first, last, alone


def pairs(w, sizes=SIZES):
    return list(zip(chunks_of(w["quals"], sizes), chunks_of(w["seqs"], sizes)))


def compare(got, base, w, low=None, bad=None):
    low = w["low"] if low is None else low
    assert (got["bad_windows"] == (w["bad"] if bad is None else bad)).all(), np.flatnonzero(got["bad_windows"] != w["bad"])[:10]
    assert (got["low_complexity"] == low).all()
    for k in SAME:  # every score, of flagged and unflagged reads alike, bit for bit
        assert got[k].tobytes() == base[k].tobytes(), k
    want_pass = base["passed"] & (low == 0)
    want_child = base["child_passed"].copy()
    for i in np.flatnonzero(low):
        want_child[int(base["child_offsets"][i]):int(base["child_offsets"][i + 1])] = 0
    assert (got["passed"] == want_pass).all() and (got["child_passed"] == want_child).all()
    return want_pass, want_child


KW = dict(chunk_bytes=1 << 16, chunk_reads=16)


def test_phred_mode(ctx, world):
    w = world
    params = api.make_params(min_length=100, min_mean_q=70)
    base = ctx.score_stream(chunks_of(w["quals"], SIZES), params, **KW)
    got = ctx.score_stream(pairs(w), params, max_low_complexity=PERCENT, low_complexity_score=SCORE, **KW)
    want_pass, _ = compare(got, base, w)
    assert base["passed"].sum() > want_pass.sum() > 10  # the filter took reads that had passed, and left others
    assert min(placements(w["low"])) >= 2  # flagged reads first, last and alone in a chunk
    # slots that grow, larger chunks
    kw = dict(chunk_bytes=4096, chunk_reads=4, grow=True)
    got = ctx.score_stream(pairs(w, (40,)), params, max_low_complexity=PERCENT, low_complexity_score=SCORE, **kw)
    compare(got, ctx.score_stream(chunks_of(w["quals"], (40,)), params, **kw), w)


def test_phred_mode_with_a_screen(ctx, world):
    """one sequence plane serves both; a read may be flagged by both, and shows in both"""
    w = world
    params = api.make_params(min_length=100)
    base = ctx.score_stream(pairs(w), params, exclude=w["xs"], exclude_percent=10.0, **KW)
    got = ctx.score_stream(pairs(w), params, exclude=w["xs"], exclude_percent=10.0, max_low_complexity=PERCENT, **KW)
    compare(got, base, w)
    assert (got["hits"] == base["hits"]).all() and (got["excluded"] == base["excluded"]).all() and got["excluded"].sum() >= 5
    assert ((got["excluded"] != 0) & (got["passed"] != 0)).sum() == 0


def test_phred_mode_with_adapters_and_both(ctx, world):
    w = world
    params = api.make_params(window_size=100, min_length=100)
    for extra in (dict(), dict(exclude=w["xs"], exclude_percent=10.0)):
        base = ctx.score_stream(pairs(w), params, adapters=w["ad"], **extra, **KW)
        got = ctx.score_stream(pairs(w), params, adapters=w["ad"], max_low_complexity=PERCENT, **extra, **KW)
        _, want_child = compare(got, base, w)  # (the filter looks at the whole parent, adapter included)
        assert (got["adapter_keys"] == base["adapter_keys"]).all()
        per = np.diff(base["child_offsets"].astype(np.int64))
        assert ((per >= 1) & (w["low"] != 0)).sum() >= 5, "flagged parents with a trimmed child"
        assert base["child_passed"].sum() > want_child.sum() > 0


def test_phred_mode_split_window_q(ctx, world):
    w = world
    params = api.make_params(min_length=200)
    base = ctx.score_stream(chunks_of(w["quals"], SIZES), params, split_window_q=85, **KW)
    got = ctx.score_stream(pairs(w), params, split_window_q=85, max_low_complexity=PERCENT, **KW)
    _, want_child = compare(got, base, w)
    per = np.diff(base["child_offsets"].astype(np.int64))
    assert ((per >= 2) & (w["low"] != 0)).sum() >= 2, "a flagged parent with children"
    assert base["child_passed"].sum() > want_child.sum() > 0


def test_kmer_mode_trim_split(ctx, world):
    w = world
    params = api.make_params(min_length=100, trim=True, split=100)
    base = ctx.score_stream(chunks_of(w["seqs"], SIZES), params, kmers=w["gs"], **KW)
    got = ctx.score_stream(chunks_of(w["seqs"], SIZES), params, kmers=w["gs"], max_low_complexity=PERCENT, **KW)
    _, want_child = compare(got, base, w)
    per = np.diff(base["child_offsets"].astype(np.int64))
    assert ((per >= 2) & (w["low"] != 0)).sum() >= 5, "the G-junk-G chimeras: children of a flagged parent"
    assert base["child_passed"].sum() > want_child.sum() > 0


def test_percent_and_score_move_the_decision(ctx, world):
    w = world
    params = api.make_params(min_length=1)
    lengths = [len(s) for s in w["seqs"]]
    got = ctx.score_stream([(w["quals"], w["seqs"])], params, chunk_bytes=1 << 20, chunk_reads=256, max_low_complexity=95.0)
    low95 = model.flagged_many(w["bad"], lengths, 95.0)
    assert (got["low_complexity"] == low95).all() and (got["bad_windows"] == w["bad"]).all() and 0 < low95.sum() < w["low"].sum()
    assert (got["passed"] == ((low95 == 0) & (np.array(lengths) >= 1))).all()
    bad300 = model.bad_many(w["seqs"], 300)
    got = ctx.score_stream([(w["quals"], w["seqs"])], params, chunk_bytes=1 << 20, chunk_reads=256, max_low_complexity=PERCENT, low_complexity_score=300)
    assert (got["bad_windows"] == bad300).all() and (got["low_complexity"] == model.flagged_many(bad300, lengths, PERCENT)).all()
    assert bad300.sum() < w["bad"].sum()


def test_call_order_and_arguments(ctx, world):
    L, w = ctx.L, world
    params = api.make_params()
    pipe = C.c_void_p()
    ctx._check(L.flx_pipeline_create(ctx.h, None, C.byref(params), 1 << 16, 64, C.byref(pipe)))
    try:
        assert L.flx_pipeline_set_complexity(pipe, 0.0, 20) == 1 and L.flx_pipeline_set_complexity(pipe, 100.5, 20) == 1
        assert L.flx_pipeline_set_complexity(pipe, 50.0, 9) == 1 and L.flx_pipeline_set_complexity(pipe, 50.0, 301) == 1
        bp, fp = C.c_void_p(), C.c_void_p()
        assert L.flx_pipeline_complexity(pipe, C.byref(bp), C.byref(fp)) == 4  # FLX_ERR_STATE: no filter on this pipeline
        buf, cb, cr = C.c_void_p(), C.c_uint64(), C.c_uint64()
        ctx._check(L.flx_pipeline_next_buffer(pipe, C.byref(buf), C.byref(cb), C.byref(cr)))
        assert L.flx_pipeline_set_complexity(pipe, 50.0, 20) == 4  # after next_buffer
        plane, offsets, lengths = api.pack_reads([w["quals"][0]])
        C.memmove(buf, plane.ctypes.data, plane.nbytes)
        ctx._check(L.flx_pipeline_submit(pipe, plane.nbytes, offsets.ctypes.data, lengths.ctypes.data, 1))
        assert L.flx_pipeline_set_complexity(pipe, 50.0, 20) == 4  # after a submit
        s, n = api.Scores(), C.c_uint64()
        ctx._check(L.flx_pipeline_finish(pipe, C.byref(s), C.byref(n)))
        assert n.value == 1
    finally:
        L.flx_pipeline_destroy(pipe)


def test_without_the_filter_nothing_of_it_runs(ctx, world):
    """the launches of a pipeline without the flag: none carries the filter's names; with it, two more a chunk and nothing else"""
    w = world
    params = api.make_params(min_length=500)
    ctx.timing_enable(True)
    try:
        ctx.timing_reset()
        base = ctx.score_stream(chunks_of(w["quals"], (16,)), params, chunk_bytes=1 << 16, chunk_reads=64)
        _, all_launches = ctx.timing_get("")
        assert ctx.timing_get("flx_complexity")[1] == 0 and all_launches > 0
        ctx.timing_reset()
        got = ctx.score_stream(pairs(w, (16,)), params, chunk_bytes=1 << 16, chunk_reads=64, max_low_complexity=PERCENT)
        chunks = len(chunks_of(w["quals"], (16,)))
        assert ctx.timing_get("flx_complexity")[1] == 2 * chunks  # "flx_complexity" and "flx_complexity_apply", once a chunk
        assert ctx.timing_get("")[1] == all_launches + 2 * chunks  # and nothing else moved
    finally:
        ctx.timing_enable(False)
    compare(got, base, w)
