"""flx_adapter_cuts and flx_score_batch_adapters against tests/_adapters_model.py, for equality.

The bytes between the reads of a plane (the padding up to 16, and any gap behind it) are filled with an adapter's own sequence: a
kernel that read a base beyond a read's last would find an adapter there.  Every call goes through the host-array form, which
prefills the device keys with 0xA5: a kernel that wrote nothing cannot pass.

A sequence always brings its reverse complement, so pattern counts are even: where the wave edges ask for 63, 64 and 65, the sets
have 31, 32, 33 and 63, 64, 65 SEQUENCES (62 .. 130 patterns: a read end's patterns straddle one and two wave edges), 1 and 2
sequences are the smallest sets and 128 sequences the 256 patterns."""
import ctypes as C

import numpy as np
import pytest

import _adapters_cases as cases
import _adapters_model as model
from filtlong_amd import api, synth
from filtlong_amd._lib import Scores

pytestmark = pytest.mark.gpu

EDGE_M = (12, 31, 32, 33, 63, 64)


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


def check(ctx, seqs, errors, window, reads, order=None, twice=False):
    pats = model.patterns(seqs)
    plane, offsets, lengths = cases.pack(reads, fill=bytes(seqs[0]).upper())
    ad = api.Adapters(seqs, errors=errors, window=window)
    assert len(ad) == len(pats)
    got = ctx.adapter_cuts(plane, offsets, lengths, ad, order=order)
    want = model.keys_of(reads, window, pats, errors)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, [(int(i), len(reads[i]), got[i].tolist(), want[i].tolist()) for i in bad[:8]]
    if twice:
        assert (ctx.adapter_cuts(plane, offsets, lengths, ad, order=order) == want).all()
    ad.close()
    return want


@pytest.fixture(scope="module")
def edge_set():
    rng = np.random.default_rng(41)
    seqs = [cases.random_adapter(rng, m) for m in EDGE_M]
    return seqs, cases.reads_for(rng, seqs, 150) + cases.reads_for(rng, seqs[3:], 150)


@pytest.fixture(scope="module")
def edge_want(edge_set):
    seqs, reads = edge_set
    return model.keys_of(reads, 150, model.patterns(seqs), 20)


def test_pattern_lengths_and_placements(ctx, edge_set, edge_want):
    """patterns of 12, 31, 32, 33, 63 and 64 bases at W = 150, E = 20 over every placement and edge length; and a second call"""
    seqs, reads = edge_set
    want = check(ctx, seqs, 20, 150, reads, twice=True)
    assert (want == edge_want).all()
    hit = want >> 8
    assert (hit[:, 0] > 0).sum() > 20 and (hit[:, 1] > 0).sum() > 20 and ((hit[:, 0] == 0) & (hit[:, 1] == 0)).sum() > 5
    assert (hit == 150).any()  # an occurrence that ends exactly at W


@pytest.mark.parametrize("how", ["descending", "ascending", "random"])
def test_orders(ctx, edge_set, edge_want, how):
    seqs, reads = edge_set
    plane, offsets, lengths = cases.pack(reads, fill=seqs[0])
    order = np.argsort(lengths, kind="stable").astype(np.uint32)
    if how == "descending":
        order = order[::-1].copy()
    elif how == "random":
        order = np.random.default_rng(2).permutation(len(reads)).astype(np.uint32)
    ad = api.Adapters(seqs, errors=20, window=150)
    assert (ctx.adapter_cuts(plane, offsets, lengths, ad, order=order) == edge_want).all()
    for broken in (np.zeros(len(reads), dtype=np.uint32), np.arange(1, len(reads) + 1, dtype=np.uint32)):
        with pytest.raises(api.FlxError) as e:
            ctx.adapter_cuts(plane, offsets, lengths, ad, order=broken)
        assert e.value.code == 1
    with pytest.raises(api.FlxError):  # a read that leaves the plane
        ctx.adapter_cuts(plane, offsets, np.where(np.arange(len(reads)) == len(reads) - 1, lengths + 64, lengths), ad)
    with pytest.raises(api.FlxError):  # an offset off the 16-byte grid
        ctx.adapter_cuts(plane, offsets + np.uint64(1), lengths, ad)


@pytest.mark.parametrize("n_seqs", [1, 2, 31, 32, 33, 63, 64, 65, 128])
def test_pattern_counts(ctx, n_seqs):
    rng = np.random.default_rng(n_seqs)
    seqs = [cases.random_adapter(rng, int(rng.integers(12, 21))) for _ in range(n_seqs)]
    reads = [b"", cases.random_seq(rng, 11), cases.random_seq(rng, 200)]
    for pick in (0, n_seqs - 1, n_seqs // 2, int(rng.integers(0, n_seqs))):
        s = seqs[pick]
        reads.append(cases.random_seq(rng, int(rng.integers(0, 8))) + s + cases.random_seq(rng, 90) + model.revcomp(seqs[n_seqs - 1 - pick]))
        reads.append(cases.random_seq(rng, 60) + cases.substitute(rng, s, 2) + cases.random_seq(rng, int(rng.integers(0, 5))))
    want = check(ctx, seqs, 20, 32, reads)
    assert (want[3:] > 0).sum() >= 8
    assert n_seqs < 3 or len(set((want[want > 0] & 255).tolist())) > 2  # several patterns decide somewhere


@pytest.mark.parametrize("window,errors", [(1, 20), (16, 0), (16, 40), (150, 0), (150, 40)])
def test_windows_and_errors(ctx, window, errors):
    rng = np.random.default_rng(1000 * window + errors)
    seqs = [cases.LIGATION, cases.random_adapter(rng, 12), cases.random_adapter(rng, 16)]
    want = check(ctx, seqs, errors, window, cases.reads_for(rng, seqs, window))
    if window == 150:
        assert (want > 0).any()


def test_widest_window_and_long_reads(ctx):
    """W = 1024 with 64-base patterns, a read of 1030 bases (a 128-byte start) and one of 300 kbp"""
    rng = np.random.default_rng(77)
    seqs = [cases.random_adapter(rng, 64), cases.random_adapter(rng, 63), cases.LIGATION]
    long_read = cases.random_seq(rng, 900) + seqs[0] + cases.random_seq(rng, 300000 - 1030) + model.revcomp(seqs[1]) + cases.random_seq(rng, 3)
    reads = [long_read, cases.random_seq(rng, 960) + seqs[0] + cases.random_seq(rng, 6),           # ends exactly at W; 1030 bases
             cases.random_seq(rng, 961) + seqs[0] + cases.random_seq(rng, 1100),                   # ends at W + 1
             cases.random_seq(rng, 1500) + cases.indel(rng, cases.substitute(rng, seqs[1], 5), 2) + cases.random_seq(rng, 700),
             cases.random_seq(rng, 1023), cases.random_seq(rng, 1025) + cases.LIGATION, cases.random_seq(rng, 2047), b"N" * 1024 + seqs[2]]
    want = check(ctx, seqs, 20, 1024, reads)
    assert len(reads[1]) == 1030 and want[1, 0] == (1024 << 8) | 0 and want[0, 0] >> 8 == 964 and want[0, 1] >> 8 == 66


def test_ties(ctx):
    """two patterns that end at the same j: the pattern index decides; a homopolymer, where every j ties: the largest wins"""
    x = b"GATTACAGATTACACCGTAG"
    seqs = [x, x[4:], b"A" * 12]
    reads = [x + b"C" * 30, b"A" * 40 + b"CCGG" * 10, b"C" + b"A" * 200, b"CCGG" * 10 + model.revcomp(x)]
    want = check(ctx, seqs, 0, 150, reads)
    assert want[0, 0] == (20 << 8) | 2 and want[1, 0] == (40 << 8) | 4 and want[2, 0] == (150 << 8) | 4 and want[3, 1] == (20 << 8) | 3


def test_what_create_refuses():
    good = b"ACGTACGTACGTAA"
    for seqs, errors, window in (([b"ACGTACGTACG"], 20, 150), ([b"A" * 65], 20, 150), ([b"ACGTACGTACGTNA"], 20, 150), ([good] * 129, 20, 150),
                                 ([good], 41, 150), ([good], -1, 150), ([good], 20, 0), ([good], 20, 1025), ([], 20, 150)):
        with pytest.raises(api.FlxError) as e:
            api.Adapters(seqs, errors=errors, window=window)
        assert e.value.code == 1
    assert len(api.Adapters([good.lower()] * 128, errors=40, window=1024)) == 256


# ---- flx_score_batch_adapters ------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def scored():
    rng = np.random.default_rng(8)
    seqs = [cases.LIGATION, cases.random_adapter(rng, 16)]
    reads = cases.reads_for(rng, seqs, 60) + [cases.random_seq(rng, 5000), cases.LIGATION + cases.random_seq(rng, 7000) + model.revcomp(seqs[1])]
    quals = [synth.qual_read(300 + i, len(r)).tobytes() if len(r) else b"" for i, r in enumerate(reads)]
    return seqs, reads, quals


def test_score_batch_adapters(ctx, scored):
    seqs, reads, quals = scored
    window, errors = 60, 20
    keys = model.keys_of(reads, window, model.patterns(seqs), errors)
    splane, offsets, lengths = cases.pack(reads, fill=seqs[0])
    qplane, qoff, _ = cases.pack(quals)
    assert (qoff == offsets).all()
    params = api.make_params(window_size=50, min_length=200, min_mean_q=5.0)
    ad = api.Adapters(seqs, errors=errors, window=window)
    for order in (None, api.length_order(lengths)):
        got = ctx.score_reads(qplane, offsets, lengths, params, order=order, adapters=ad, seq_plane=splane, child_capacity=1)
        plain = ctx.score_reads(qplane, offsets, lengths, params, order=order)
        children, parents, coff = [], [], [0]
        for i, r in enumerate(reads):
            ch, first, last = model.child_of(len(r), keys[i, 0], keys[i, 1])
            assert (got["first"][i], got["last"][i]) == (first, last), i
            children += ch
            parents += [i] * len(ch)
            coff.append(len(children))
        assert got["child_offsets"].tolist() == coff and got["child_ranges"].tolist() == [list(c) for c in children]
        assert any(f == -1 for f in got["first"]) and len(children) > 10
        # a parent keeps its own scores; one with nothing left fails
        assert (got["mean_q"].view(np.uint64) == plain["mean_q"].view(np.uint64)).all()
        assert (got["window_q"].view(np.uint64) == plain["window_q"].view(np.uint64)).all()
        gone = got["first"] == -1
        assert (got["passed"][gone] == 0).all() and (got["passed"][~gone] == plain["passed"][~gone]).all()
        # a child gets the bits flx_score_batch gives its quality substring
        subs = [quals[p][s:e] for p, (s, e) in zip(parents, children)]
        cplane, coffs, clens = cases.pack(subs)
        alone = ctx.score_reads(cplane, coffs, clens, params)
        assert (got["child_mean_q"].view(np.uint64) == alone["mean_q"].view(np.uint64)).all()
        assert (got["child_window_q"].view(np.uint64) == alone["window_q"].view(np.uint64)).all()
        assert (got["child_passed"] == alone["passed"]).all() and 0 < alone["passed"].sum() < len(subs)
    ad.close()


def test_score_batch_adapters_capacity(ctx, scored):
    seqs, reads, quals = scored
    keys = model.keys_of(reads, 60, model.patterns(seqs), 20)
    needed = sum(len(model.child_of(len(r), k[0], k[1])[0]) for r, k in zip(reads, keys))
    splane, offsets, lengths = cases.pack(reads, fill=seqs[0])
    qplane, _, _ = cases.pack(quals)
    params = api.make_params(window_size=50)
    ad = api.Adapters(seqs, errors=20, window=60)
    n = len(reads)
    mean, win, passed = np.zeros(n), np.zeros(n), np.zeros(n, dtype=np.uint8)
    coff = np.zeros(n + 1, dtype=np.uint64)
    cap = needed - 1
    cr, cm, cw, cp = np.zeros(2 * cap, dtype=np.int32), np.zeros(cap), np.zeros(cap), np.zeros(cap, dtype=np.uint8)
    s = Scores()
    s.mean_q, s.window_q, s.passed, s.child_offsets = mean.ctypes.data, win.ctypes.data, passed.ctypes.data, coff.ctypes.data
    s.child_ranges, s.child_mean_q, s.child_window_q, s.child_passed, s.child_capacity = cr.ctypes.data, cm.ctypes.data, cw.ctypes.data, cp.ctypes.data, cap
    rc = ctx.L.flx_score_batch_adapters(ctx.h, ad.h, qplane.ctypes.data, splane.ctypes.data, qplane.nbytes, offsets.ctypes.data, lengths.ctypes.data,
                                        None, n, C.byref(params), C.byref(s))
    assert rc == 5 and s.n_children == needed  # FLX_ERR_CAPACITY with the count needed
    for bad in (api.make_params(window_size=50, trim=True), api.make_params(window_size=50, split=100)):
        with pytest.raises(api.FlxError) as e:
            ctx.score_reads(qplane, offsets, lengths, bad, adapters=ad, seq_plane=splane)
        assert e.value.code == 1
    ad.close()
