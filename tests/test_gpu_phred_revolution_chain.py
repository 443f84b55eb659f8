"""The static window-250 Phred kernel's fast ring revolutions (a wave folds the RR = 5 rounds of a ring revolution straight-line,
without a compare or branch between them, while 64 (rb + RR) <= Lmin; the per-round code takes the rest of the group) against the
oracle, bit for bit.  The batch is scored WITHOUT the length order, so a wave is 64 consecutive reads and every block of 64 below
decides its wave's Lmin: with H = 4 prologue rounds the revolution that starts at round 4 is fast from Lmin = 576 on, the following
ones from 896, 1216, ...  The lengths around 640, 960 and 1280 are where a chain that crosses the rounds would switch (it needs one
more whole round behind the revolution: profiles/revolution_chain.md); they stay as cases of rounds behind a fast revolution."""
import numpy as np
import pytest

import _oracle
from filtlong_amd import api
from test_gpu_phred_fold_schedule import _regs_name, _same, _select

pytestmark = pytest.mark.gpu

# one length per block of 64: the thresholds of the first three fast revolutions and one below and above them; round (64 k) and
# chunk (128 k) boundaries inside and just behind a fast revolution; several revolutions, starting on both halves of the slot
EQUAL_LENGTHS = sorted(set([575, 576, 577, 895, 896, 897, 1215, 1216, 1217]
                           + [639, 640, 641, 959, 960, 961, 1279, 1280, 1281]
                           + [64 * k + e for k in range(10, 17) for e in (-1, 0, 1)]
                           + [128 * k + e for k in range(5, 9) for e in (-1, 1)]
                           + [2000, 3000]))
LAST_BLOCK = 37


def _blocks():
    """(name, lengths of the block's reads, repeated byte or None)"""
    b = [("equal %d" % L, [L] * 64, None) for L in EQUAL_LENGTHS]
    b.append(("one byte 3000", [3000] * 64, 75))
    b.append(("3000 and one 500", [3000] * 7 + [500] + [3000] * 56, None))    # Lmin keeps the wave off the fast path
    b.append(("3000 and one 600", [3000] * 20 + [600] + [3000] * 43, None))   # one fast revolution (rounds 4..8), then masked rounds
    b.append(("3000 and one 700", [3000] * 41 + [700] + [3000] * 22, None))   # while the other lanes go on: from round 9 / round 10 on
    b.append(("1280..1343", list(range(1280, 1344)), None))                   # every lane ends in the round behind the last fast one
    b.append(("last block", [1500] * LAST_BLOCK, None))
    return b


_CACHE = {}


def _batch():
    if "quals" not in _CACHE:
        rng = np.random.RandomState(2507)
        quals = []
        for _, lens, byte in _blocks():
            for L in lens:
                q = np.full(L, byte, dtype=np.uint8) if byte is not None else rng.randint(33, 127, size=L).astype(np.uint8)
                quals.append(q.tobytes())
        _CACHE["quals"] = quals
        _CACHE["packed"] = api.pack_reads(quals)
        p = _oracle.make_params(window_size=250)
        rows = [_oracle.score_read(None, q, p) for q in quals]
        _CACHE["want"] = {"mean_q": np.array([r["mean_q"] for r in rows]), "window_q": np.array([r["window_q"] for r in rows]),
                          "passed": np.array([r["passed"] for r in rows], dtype=np.uint8)}
    return _CACHE["quals"]


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


def _score(ctx):
    _batch()
    plane, offsets, lengths = _CACHE["packed"]
    return ctx.score_reads(plane, offsets, lengths, api.make_params(window_size=250), order=None)


def test_the_batch_holds_what_it_should():
    blocks = _blocks()
    lens = [len(q) for q in _batch()]
    assert all(len(b[1]) == 64 for b in blocks[:-1]) and len(blocks[-1][1]) == LAST_BLOCK < 64
    assert len(lens) == 64 * (len(blocks) - 1) + LAST_BLOCK and max(lens) == 3000 and len(lens) < 4000
    firsts = lens[0::64]  # every block starts at a multiple of 64: it is one wave
    assert firsts[:len(EQUAL_LENGTHS)] == EQUAL_LENGTHS
    for L in (575, 576, 577, 895, 896, 897, 1215, 1216, 1217, 639, 640, 641, 703, 704, 705, 959, 960, 961, 1023, 1024, 1025, 1279, 1280, 1281, 2000, 3000):
        assert L in EQUAL_LENGTHS
    for name, want_min in (("3000 and one 500", 500), ("3000 and one 600", 600), ("3000 and one 700", 700), ("1280..1343", 1280)):
        i = [b[0] for b in blocks].index(name)
        assert min(lens[64 * i:64 * i + 64]) == want_min
    i = [b[0] for b in blocks].index("one byte 3000")
    assert len(set(_batch()[64 * i])) == 1


@pytest.mark.parametrize("tables", ["plain", "private"])
def test_fast_revolutions_against_the_oracle(ctx, tables, monkeypatch):
    _select(monkeypatch, tables, "static")
    o = _score(ctx)
    assert ctx.last_phred_kernel() == _regs_name(tables)
    _same(o, _CACHE["want"], "ws 250 %s static" % tables)


@pytest.mark.parametrize("tables", ["plain", "private"])
def test_static_and_generic_agree(ctx, tables, monkeypatch):
    """The generic kernel (FLX_PHRED_FUNNEL=runtime) has no fast revolution."""
    _select(monkeypatch, tables, "static")
    st = _score(ctx)
    assert ctx.last_phred_kernel() == _regs_name(tables)
    _select(monkeypatch, tables, "runtime")
    ge = _score(ctx)
    assert ctx.last_phred_kernel() == _regs_name(tables)
    _same(ge, st, "ws 250 %s generic against static" % tables)
    _same(ge, _CACHE["want"], "ws 250 %s generic" % tables)
