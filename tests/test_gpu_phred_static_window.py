"""Register-history Phred kernel: the static-window instantiation (window 250: ws % 16 at compile time, trailing bytes selected
from the ring dwords, no funnel) against the oracle, bit for bit, and against the generic kernel (FLX_PHRED_FUNNEL=runtime);
and the placement of every one of a chunk's eight LDS-DMA destinations."""
import numpy as np
import pytest

import _oracle
from filtlong_amd import api

pytestmark = pytest.mark.gpu

EDGE_LENGTHS = [0, 1, 249, 250, 251, 255, 256, 257, 265, 266, 267, 319, 320, 321, 383, 384, 385, 511, 512, 513, 639, 640, 641]


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


def _bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64)


def _same(o, want, tag):
    for f in ("mean_q", "window_q"):
        got, w = np.asarray(o[f]), want[f]
        assert (np.isnan(got) == np.isnan(w)).all(), tag + " " + f + ": NaN pattern differs"
        bad = np.nonzero((_bits(got) != _bits(w)) & ~np.isnan(w))[0]
        assert len(bad) == 0, "%s %s: %d mismatches, first at read %d: got %s want %s" % (
            tag, f, len(bad), bad[0], float(got[bad[0]]).hex(), float(w[bad[0]]).hex())
    assert (np.asarray(o["passed"]) == want["passed"]).all(), tag + " passed"


def _fastq_batch():
    """Every edge the static selects have (window, boundary piece, ring revolution, chunk ends), waves that mix reads ending in
    different chunks, and a group of full reads followed by a partly filled one."""
    rng = np.random.RandomState(250)
    lens = EDGE_LENGTHS + [int(x) for x in rng.randint(1, 3001, 200)] + [5000] * 70
    return [rng.randint(33, 127, size=L).astype(np.uint8).tobytes() for L in lens]


def _redo_batch():
    """Reads with bytes >= 128 (bank-private tables: flagged, re-scored by the redo kernel) and bytes < 33 (negative q) among
    ordinary ones."""
    rng = np.random.RandomState(251)
    quals = [rng.randint(33, 127, size=L).astype(np.uint8) for L in (250, 251, 266, 300, 513, 1000, 2000, 2500)]
    for L, lo, hi in ((251, 0, 256), (300, 0, 256), (777, 128, 256), (1500, 0, 33), (640, 0, 128), (2100, 0, 256)):
        quals.append(rng.randint(lo, hi, size=L).astype(np.uint8))
    q = rng.randint(33, 127, size=900).astype(np.uint8)
    q[0], q[449], q[-1] = 0xff, 0x80, 0x05  # single bytes at either end and in the middle
    quals.append(q)
    return [q.tobytes() for q in quals]


_BATCHES = {}
_WANT = {}


def _batch(name):
    if name not in _BATCHES:
        _BATCHES[name] = {"fastq": _fastq_batch, "redo": _redo_batch}[name]()
    return _BATCHES[name]


def _oracle_scores(name, quals, ws):
    """The oracle's values of one batch at one window size: computed once, shared by every test and kernel variant."""
    if (name, ws) not in _WANT:
        p = _oracle.make_params(window_size=ws)
        rows = [_oracle.score_read(None, q, p) for q in quals]
        _WANT[(name, ws)] = {"mean_q": np.array([r["mean_q"] for r in rows]), "window_q": np.array([r["window_q"] for r in rows]),
                             "passed": np.array([r["passed"] for r in rows], dtype=np.uint8)}
    return _WANT[(name, ws)]


def _score(ctx, quals, ws, use_order=True):
    plane, offsets, lengths = api.pack_reads(quals)
    order = api.length_order(lengths) if use_order else None
    return ctx.score_reads(plane, offsets, lengths, api.make_params(window_size=ws), order=order)


def _select(monkeypatch, tables, funnel):
    monkeypatch.setenv("FLX_PHRED_LONG_MIN", "0")  # keeps the cooperative long-read path out
    monkeypatch.setenv("FLX_PHRED_TABLES", tables)
    if funnel == "runtime":
        monkeypatch.setenv("FLX_PHRED_FUNNEL", "runtime")
    else:
        monkeypatch.delenv("FLX_PHRED_FUNNEL", raising=False)


def _kernel_name(tables):
    return "flx_score_phred_regs_private" if tables == "private" else "flx_score_phred_regs"


@pytest.mark.parametrize("funnel", ["static", "runtime"])
@pytest.mark.parametrize("tables", ["plain", "private"])
def test_window_250_static_and_generic_match_the_oracle(ctx, tables, funnel, monkeypatch):
    """All four ways equal the oracle bit for bit, hence each other; the names reported to the host do not change."""
    _select(monkeypatch, tables, funnel)
    quals = _batch("fastq")
    want = _oracle_scores("fastq", quals, 250)
    for use_order in (True, False):
        o = _score(ctx, quals, 250, use_order)
        assert ctx.last_phred_kernel() == _kernel_name(tables)
        _same(o, want, "ws 250 %s %s order=%s" % (tables, funnel, use_order))


@pytest.mark.parametrize("funnel", ["static", "runtime"])
@pytest.mark.parametrize("tables", ["plain", "private"])
def test_window_250_redo_and_zero_entry_masking(ctx, tables, funnel, monkeypatch):
    """Bytes >= 128 and < 33: the private tables' redo path and the masking of ended reads give the oracle's values."""
    _select(monkeypatch, tables, funnel)
    quals = _batch("redo")
    _same(_score(ctx, quals, 250), _oracle_scores("redo", quals, 250), "redo ws 250 %s %s" % (tables, funnel))


@pytest.mark.parametrize("ws", [240, 249, 251, 256])
def test_neighbouring_windows_take_the_generic_kernel(ctx, ws, monkeypatch):
    """Only window 250 has a static instantiation: its neighbours (B = 0, 9, 11 and A = 16) still match the oracle."""
    quals = _batch("fastq")
    want = _oracle_scores("fastq", quals, ws)
    for tables in ("plain", "private"):
        _select(monkeypatch, tables, "static")
        o = _score(ctx, quals, ws)
        assert ctx.last_phred_kernel() == _kernel_name(tables)
        _same(o, want, "ws %d %s" % (ws, tables))


def _labelled_reads(n, L):
    """Every 16-byte piece carries its read and piece number (remapped into 33..126): a DMA that lands a piece at another
    place of the slot gives another read's or another piece's bytes."""
    reads = []
    for r in range(n):
        q = np.empty(L, dtype=np.uint8)
        for k in range(L):
            p = k >> 4
            q[k] = 33 + (r if (k & 15) == 0 else p if (k & 15) == 1 else (r * 31 + p * 17 + (k & 15) * (3 + (r + p) % 7)) % 94)
        reads.append(q.tobytes())
    return reads


@pytest.mark.parametrize("L", [129, 128])
def test_dma_destinations_and_both_slot_halves(ctx, L, monkeypatch):
    """One full wave of 64 equal reads, window 16: with 129 bases chunk 0 exists whole for every lane and chunk 1 holds one
    piece per read; with 128 bases chunk 0 is itself the last chunk.  All eight DMA destinations and both halves of the slot
    are in use."""
    quals = _labelled_reads(64, L)
    want = _oracle_scores("labelled%d" % L, quals, 16)
    for tables in ("plain", "private"):
        _select(monkeypatch, tables, "static")
        _same(_score(ctx, quals, 16), want, "labelled L %d %s" % (L, tables))


def test_unknown_funnel_value_is_refused(ctx, monkeypatch):
    monkeypatch.setenv("FLX_PHRED_LONG_MIN", "0")
    monkeypatch.setenv("FLX_PHRED_FUNNEL", "static")
    with pytest.raises(api.FlxError, match="FLX_PHRED_FUNNEL"):
        _score(ctx, _labelled_reads(2, 40), 250)
