"""flx_complexity_bad (csrc/complexity.hip) against tests/_complexity_model.py for equality, per read: the edge cases of the host
program (tests/test_complexity_host.py), the borderline windows, and a mixed batch of about 200 reads — with order NULL and a
permutation, at T = 10, 20, 37 and 300; a read of three spans and 17 bases whose bad windows are summed by several waves, a read of
no base between two others, two calls that must agree (nothing is accumulated), and the score's range."""
import numpy as np
import pytest

import _complexity_cases as cases
import _complexity_model as model
from filtlong_amd import api

pytestmark = pytest.mark.gpu
SCORES = (10, 20, 37, 300)


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def batch():
    """the reads, packed once, and the model's answers at every T"""
    rng = np.random.default_rng(2024)
    span = api.complexity_span()
    reads = cases.edge_reads(rng, span)
    for T in (10, 20, 300):
        reads += cases.borderline_reads(np.random.default_rng(T), T)
    reads += cases.mixed_batch(rng, 200)
    long_one = model.repeat(rng, 3, span + 500) + model.random_seq(rng, span) + model.repeat(rng, 5, span - 500 + 17)
    assert len(long_one) == 3 * span + 17
    reads += [model.random_seq(rng, 300), b"", model.repeat(rng, 2, 300), long_one]
    plane, offsets, lengths = api.pack_reads(reads)
    want = {T: model.bad_many(reads, T) for T in SCORES}
    return {"reads": reads, "plane": plane, "offsets": offsets, "lengths": lengths, "want": want, "span": span}


def check(got, want, reads):
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, (len(bad), [(int(i), len(reads[i]), int(got[i]), int(want[i])) for i in bad[:10]])


def test_constants():
    assert api.complexity_window() == 64
    span = api.complexity_span()
    assert span % 64 == 0 and span >= 64 * 64  # every lane of a wave owns at least a window's length of starts


@pytest.mark.parametrize("T", SCORES)
def test_equals_model(ctx, batch, T):
    b = batch
    got = ctx.complexity_bad(b["plane"], b["offsets"], b["lengths"], score=T)
    check(got, b["want"][T], b["reads"])
    order = np.random.default_rng(T).permutation(len(b["reads"])).astype(np.uint32)
    check(ctx.complexity_bad(b["plane"], b["offsets"], b["lengths"], score=T, order=order), b["want"][T], b["reads"])
    check(ctx.complexity_bad(b["plane"], b["offsets"], b["lengths"], score=T, order=api.length_order(b["lengths"])), b["want"][T], b["reads"])
    if T < 300:
        assert (got > 0).sum() > len(got) // 3 and (got == 0).sum() > len(got) // 8


def test_long_read_is_summed_across_spans(ctx, batch):
    b = batch
    got = ctx.complexity_bad(b["plane"], b["offsets"], b["lengths"])
    span = b["span"]
    assert len(b["reads"][-1]) == 3 * span + 17 and got[-1] == b["want"][20][-1]
    assert 2 * span - 300 < got[-1] < 2 * span + 100  # the repeats at both ends, not the random middle
    assert got[-3] == 0 and len(b["reads"][-3]) == 0 and got[-2] == 300 - 63 and got[-4] == b["want"][20][-4]


def test_two_calls_agree(ctx, batch):
    b = batch
    first = ctx.complexity_bad(b["plane"], b["offsets"], b["lengths"], score=20)
    again = ctx.complexity_bad(b["plane"], b["offsets"], b["lengths"], score=20)
    assert (first == again).all() and (first == b["want"][20]).all()


def test_decision_on_integers(batch):
    b = batch
    for percent in (0.5, 50.0, 100.0):
        want = model.flagged_many(b["want"][20], b["lengths"], percent)
        assert (api.complexity_flagged(b["want"][20], b["lengths"], percent) == want).all()
    assert api.complexity_flagged([0, 1, 1], [63, 64, 65], 100.0).tolist() == [0, 1, 0]


@pytest.mark.parametrize("score", [9, 301])
def test_score_out_of_range(ctx, batch, score):
    b = batch
    with pytest.raises(api.FlxError) as e:
        ctx.complexity_bad(b["plane"], b["offsets"], b["lengths"], score=score)
    assert e.value.code == 1  # FLX_ERR_INVALID
