"""flx_endtrim_cuts on the GPU against tests/_endtrim_model.py, bit for bit: the lengths on the edges of a lane's run, of a step and of
the span; one read of five spans whose head and tail maxima lie in the first, a middle and the last span; reads that are all junk and
all good; junk in the middle only; the tie cases (a base that weighs exactly zero, maxima met again exactly behind a span's edge: the
earlier one wins); `order` NULL and a permutation; outputs that start as 0xA5 are fully written; any byte."""
import numpy as np
import pytest

import _endtrim_cases as cases
import _endtrim_model as model
from filtlong_amd import api

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def span():
    s = api.endtrim_span()
    assert s % 1024 == 0 and s >= 10240  # whole steps of a wave, and a 10 kbp read is one span
    return s


def gpu_cuts(ctx, reads, t, order=None):
    plane, offsets, lengths = api.pack_reads(reads)
    got = ctx.endtrim_cuts(plane, offsets, lengths, t, order=order)
    assert got.shape == (len(reads), 2) and got.dtype == np.uint32
    return got


def check(ctx, reads, t, order=None):
    got, want = gpu_cuts(ctx, reads, t, order), model.batch_cuts(reads, t)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert len(bad) == 0, [(int(i), len(reads[i]), got[i].tolist(), want[i].tolist()) for i in bad[:8]]
    return got


def test_the_tie_threshold_is_a_table_entry():
    e = api.qsplit_table()
    assert int(e[43]) == cases.T_PLUS == 429496730 and api.qsplit_threshold(90) == cases.T90 == cases.T_PLUS - 1
    assert int(e[33]) == cases.E_BANG and int(e[73]) == cases.E_I


@pytest.mark.parametrize("t", [cases.T90, cases.T_PLUS, 42949672, 0, 2**32 - 1])
def test_edge_lengths(ctx, span, t):
    reads = cases.edge_reads(np.random.default_rng(5), span)
    assert sorted(set(len(r) for r in reads)) == sorted(cases.edge_lengths(span))
    got = check(ctx, reads, t)
    assert tuple(got[0]) == (0, 0)  # no base
    if t == cases.T90:
        assert (got[:, 0] > 0).sum() > 5 and (got[:, 1] > 0).sum() > 5


def test_five_spans_each_end_in_every_span(ctx, span):
    reads = [cases.five_spans(span, where, side) for side in (0, 1) for where in (0, 2, 4)]
    got = check(ctx, reads, cases.T90)
    for k, (side, where) in enumerate([(s, w) for s in (0, 1) for w in (0, 2, 4)]):
        at = int(got[k, 0]) if side == 0 else len(reads[k]) - int(got[k, 1])
        assert at // span == where, (side, where, got[k])


def test_all_junk_all_good_and_junk_in_the_middle(ctx, span):
    rng = np.random.default_rng(8)
    junk = [cases.rand_bytes(rng, n, 33, 38) for n in (1, 40, 1025, span + 7)]
    good = [cases.rand_bytes(rng, n, ord("?"), ord("I")) for n in (1, 40, 1025, span + 7)]
    reads = junk + good + [cases.middle_junk(True), cases.middle_junk(False)]
    got = check(ctx, reads, cases.T90)
    for k, r in enumerate(junk):
        assert tuple(got[k]) == (len(r), len(r))
    assert (got[4:8] == 0).all()
    assert got[8, 0] == 230 and tuple(got[9]) == (0, 0)  # the stretch outweighs the flank, or does not


def test_ties(ctx, span):
    flat = cases.flat_reads(np.random.default_rng(7), span)
    got = check(ctx, flat, cases.T_PLUS)
    assert tuple(got[0]) == (0, 0)  # all '+'
    assert got[2, 0] == 3 and got[3, 1] == 3  # !!! +++++ IIIIIIIIII, and its mirror image
    ties = cases.span_edge_ties(span)
    cuts = {}
    for t in (cases.T_MID, cases.T_PLUS):
        idx = [i for i, (_, tt) in enumerate(ties) if tt == t]
        g = check(ctx, [ties[i][0] for i in idx], t)
        cuts.update({i: g[k] for k, i in enumerate(idx)})
    for idx, comp, value in cases.span_edge_tie_answers(span):
        assert int(cuts[idx][comp]) == value, (idx, comp, cuts[idx])


def test_order_and_prefilled_outputs(ctx, span):
    rng = np.random.default_rng(11)
    reads = cases.mixed_batch(rng, 150, 3000) + [cases.ont_like(rng, 2 * span + 300, 500, 900), b"", cases.ont_like(rng, span, 0, 0)]
    want = model.batch_cuts(reads, cases.T90)
    plain = check(ctx, reads, cases.T90)
    perm = rng.permutation(len(reads)).astype(np.uint32)
    by_length = api.length_order(api.pack_reads(reads)[2])
    for order in (perm, by_length):
        assert (check(ctx, reads, cases.T90, order=order) == plain).all()
    # (Context.endtrim_cuts hands over an output of 0xA5A5A5A5 and the library's own staging starts as 0xA5 too)
    assert (plain != 0xA5A5A5A5).all() and (want[:, 0] > 0).sum() > 50 and (want == 0).all(axis=1).sum() > 10


def test_any_byte(ctx):
    reads = cases.any_bytes(np.random.default_rng(6))
    for t in (cases.T90, cases.T_PLUS, 2**32 - 1):
        check(ctx, reads, t)


def test_argument_checks(ctx):
    plane, offsets, lengths = api.pack_reads([b"IIII!!"])
    with pytest.raises(api.FlxError):
        ctx.endtrim_cuts(plane, offsets, lengths, 2**32)
    assert ctx.endtrim_cuts(plane, offsets[:0], lengths[:0], cases.T90).shape == (0, 2)
