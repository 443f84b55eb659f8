"""Phred folds after the change of their issue schedule (one counted wait per base in fold4 / head4; in the static window-250
kernel a round's 16 folds as one chain, each computing the next group's addresses behind its own gathers): every kernel that
shares the fold against the oracle, bit for bit, on ONE batch that puts a read's end at every position of a piece, a dword and
a fold, at the end of the first ring revolution and at chunk and round boundaries, and that — scored without the length
order — makes whole rounds (chained) and rounds some lane ends in (piece by piece, masked) alternate inside a wave."""
import numpy as np
import pytest

import _oracle
from filtlong_amd import api

pytestmark = pytest.mark.gpu

LENGTHS = (list(range(250, 331)) + list(range(560, 661)) + [0, 1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 249] + [3000] * 70)
REPEAT_LENGTHS = [1, 17, 250, 251, 260, 266, 267, 281, 320, 321, 330, 576, 577, 600, 640, 641, 700, 1000, 2047, 3000]


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


def _make_batch():
    """About 400 reads: the lengths above with bytes 33..126 at random; reads of one repeated byte; reads with bytes >= 128
    and < 33 among ordinary ones (with bank-private tables they go through the redo kernel)."""
    rng = np.random.RandomState(20250)
    quals = [rng.randint(33, 127, size=L).astype(np.uint8) for L in LENGTHS]
    for i, L in enumerate(REPEAT_LENGTHS * 4):
        quals.append(np.full(L, (33, 126, 34, 75, 90, 125, 50)[i % 7], dtype=np.uint8))
    for L in [250, 251, 266, 300, 513, 1000, 2000, 2500, 3000, 329, 600, 655] + [int(x) for x in rng.randint(250, 3001, 24)]:
        quals.append(rng.randint(33, 127, size=L).astype(np.uint8))
    for L, lo, hi in ((251, 0, 256), (300, 0, 256), (777, 128, 256), (1500, 0, 33), (640, 0, 128), (2100, 0, 256), (3000, 0, 256),
                      (270, 128, 256), (610, 0, 33), (330, 0, 256)):
        quals.append(rng.randint(lo, hi, size=L).astype(np.uint8))
    for L in (900, 3000):
        q = rng.randint(33, 127, size=L).astype(np.uint8)
        q[0], q[L // 2], q[-1] = 0xff, 0x80, 0x05  # single bytes at either end and in the middle
        quals.append(q)
    return [q.tobytes() for q in quals]


_CACHE = {}


def _batch():
    if "quals" not in _CACHE:
        quals = _make_batch()
        plane, offsets, lengths = api.pack_reads(quals)
        _CACHE["quals"] = quals
        _CACHE["packed"] = (plane, offsets, lengths, api.length_order(lengths))
    return _CACHE["quals"]


def _want(ws):
    """The oracle's values of the batch at one window size: computed once, shared by every test and kernel variant."""
    if ("want", ws) not in _CACHE:
        p = _oracle.make_params(window_size=ws)
        rows = [_oracle.score_read(None, q, p) for q in _batch()]
        _CACHE[("want", ws)] = {"mean_q": np.array([r["mean_q"] for r in rows]), "window_q": np.array([r["window_q"] for r in rows]),
                                "passed": np.array([r["passed"] for r in rows], dtype=np.uint8)}
    return _CACHE[("want", ws)]


def _bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64)


def _same(o, want, tag):
    for f in ("mean_q", "window_q"):
        got, w = np.asarray(o[f]), np.asarray(want[f])
        assert (np.isnan(got) == np.isnan(w)).all(), tag + " " + f + ": NaN pattern differs"
        bad = np.nonzero((_bits(got) != _bits(w)) & ~np.isnan(w))[0]
        assert len(bad) == 0, "%s %s: %d mismatches, first at read %d: got %s want %s" % (
            tag, f, len(bad), bad[0], float(got[bad[0]]).hex(), float(w[bad[0]]).hex())
    assert (np.asarray(o["passed"]) == np.asarray(want["passed"])).all(), tag + " passed"


def _score(ctx, ws, use_order):
    _batch()
    plane, offsets, lengths, order = _CACHE["packed"]
    return ctx.score_reads(plane, offsets, lengths, api.make_params(window_size=ws), order=order if use_order else None)


def _select(monkeypatch, tables, funnel=None, kernel=None):
    monkeypatch.setenv("FLX_PHRED_LONG_MIN", "0")  # keeps the cooperative long-read path out
    monkeypatch.setenv("FLX_PHRED_TABLES", tables)
    if funnel == "runtime":
        monkeypatch.setenv("FLX_PHRED_FUNNEL", "runtime")
    else:
        monkeypatch.delenv("FLX_PHRED_FUNNEL", raising=False)
    if kernel:
        monkeypatch.setenv("FLX_PHRED_KERNEL", kernel)
    else:
        monkeypatch.delenv("FLX_PHRED_KERNEL", raising=False)


def _regs_name(tables):
    return "flx_score_phred_regs_private" if tables == "private" else "flx_score_phred_regs"


def _check_both_orders(ctx, ws, tag, kernel_name):
    want = _want(ws)
    for use_order in (True, False):
        o = _score(ctx, ws, use_order)
        assert ctx.last_phred_kernel() == kernel_name
        _same(o, want, "%s order=%s" % (tag, use_order))


def test_the_batch_holds_what_it_should():
    lens = [len(q) for q in _batch()]
    assert 380 <= len(lens) <= 420
    assert set(range(250, 331)) | set(range(560, 661)) | {0, 1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 249} <= set(lens)
    assert lens.count(3000) >= 70


@pytest.mark.parametrize("funnel", ["static", "runtime"])
@pytest.mark.parametrize("tables", ["plain", "private"])
def test_window_250_against_the_oracle(ctx, tables, funnel, monkeypatch):
    """Static (chained rounds) and generic kernel, both table variants, with and without the length order."""
    _select(monkeypatch, tables, funnel)
    _check_both_orders(ctx, 250, "ws 250 %s %s" % (tables, funnel), _regs_name(tables))


@pytest.mark.parametrize("tables", ["plain", "private"])
def test_window_250_static_and_generic_agree(ctx, tables, monkeypatch):
    for use_order in (True, False):
        _select(monkeypatch, tables, "static")
        st = _score(ctx, 250, use_order)
        _select(monkeypatch, tables, "runtime")
        _same(_score(ctx, 250, use_order), st, "ws 250 %s generic against static order=%s" % (tables, use_order))


@pytest.mark.parametrize("ws", [16, 17, 31, 40, 100, 319, 623])
@pytest.mark.parametrize("tables", ["plain", "private"])
def test_generic_instantiations_against_the_oracle(ctx, tables, ws, monkeypatch):
    """16, 12 and 8 waves per CU, B = 0 and B = 15, the first and the last instantiation (623: plain tables whatever is asked)."""
    _select(monkeypatch, tables)
    _check_both_orders(ctx, ws, "ws %d %s" % (ws, tables), _regs_name(tables if ws < 512 else "plain"))


@pytest.mark.parametrize("ws", [624, 1500])
def test_dual_slot_kernel_against_the_oracle(ctx, ws, monkeypatch):
    _select(monkeypatch, "plain")
    _check_both_orders(ctx, ws, "ws %d dual" % ws, "flx_score_phred_dual")


def test_stream_kernel_against_the_oracle(ctx, monkeypatch):
    _select(monkeypatch, "plain", kernel="stream")
    _check_both_orders(ctx, 250, "ws 250 stream", "flx_score_phred_stream")
