"""flx_adapter_marks and flx_score_batch_adapters with the middle search on, against tests/_adapters_split_model.py, for equality.

The bytes between the reads of a plane (the padding up to 16, and any gap behind it) are filled with an adapter's own sequence: a
kernel that read a base beyond a read's last would find an adapter there.  The marks come through the host-array form, whose
output is prefilled with 0xA5: every word has to be written, and every bit outside the reads has to be zero.  The children come
through flx_score_batch_adapters; their scores are held against flx_score_batch on the quality substring, bit for bit."""
import ctypes as C

import numpy as np
import pytest

import _adapters_model as model
import _adapters_split_cases as cases
from _adapters_split_checks import check, check_children, check_marks, quals_of, wanted
from filtlong_amd import api
from filtlong_amd._lib import Scores

pytestmark = pytest.mark.gpu

S = cases.PIECE_BASES


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("e2,lengths", [(0, (33, 12)), (10, (64, 31, 32, 33, 12)), (40, (64, 31))])
def test_placements(ctx, e2, lengths):
    """adapters ending on both edges of a piece and of its warm-up, straddling pieces, back to back, one base apart, merging marks,
    reverse complement, substitutions and indels; patterns of 12, 31, 32, 33 and 64 bases"""
    rng = np.random.default_rng(900 + e2)
    seqs = [cases.random_adapter(rng, m) for m in lengths]
    want = check(ctx, seqs, 20, 60, e2, cases.placements(rng, seqs, e2))
    assert sum(len(w[3]) >= 2 for w in want) > len(want) // 2
    if e2 == 0:
        assert any(e - s == 1 for w in want for s, e in w[3])  # a child of one base


def test_lengths_and_bytes(ctx):
    """reads of 0, 1, m - 1, m, S - 1, S, S + 1, 2 S, 2 S + 1 and 3 S + 5 bases; a homopolymer against a homopolymer-rich pattern,
    N, lower and mixed case, every byte value"""
    rng = np.random.default_rng(12)
    seqs = [b"AAAAAAAAAAAAAAAC", cases.LIGATION.lower(), b"A" * 12]
    reads = cases.byte_reads(rng, seqs)
    assert [len(r) for r in reads[:11]] == [0, 1, 1, 15, 16, S - 1, S, S + 1, 2 * S, 2 * S + 1, 3 * S + 5]
    want = check(ctx, seqs, 20, 150, 10, reads)
    assert want[11][2].all() and want[11][4] == -1


def test_long_read(ctx):
    """300 kbp: 293 pieces, adapters on piece boundaries far into the read; a small call behind the large one on the same context"""
    rng = np.random.default_rng(300)
    seqs = [cases.LIGATION, cases.random_adapter(rng, 28)]
    a, b = seqs
    parts = [cases.random_seq(rng, 100 * S - 10), a, cases.random_seq(rng, 50 * S - 18 - 28), model.revcomp(b), cases.random_seq(rng, 7000),
             cases.substitute(rng, a, 2)]
    long_read = b"".join(parts)
    long_read += cases.random_seq(rng, 300000 - len(long_read))
    reads = [cases.random_seq(rng, 40), long_read, cases.chimera(rng, seqs, 700, 900)]
    want = check(ctx, seqs, 20, 150, 10, reads)
    assert len(want[1][3]) == 4 and len(want[2][3]) == 2
    small = [cases.chimera(rng, seqs, 400, 500, which=1), b"ACGT"]
    assert len(check(ctx, seqs, 20, 150, 10, small)[0][3]) == 2


@pytest.mark.parametrize("n_seqs", [1, 2, 32, 128])
def test_set_sizes(ctx, n_seqs):
    """2, 4, 64 and 256 patterns: 28, 28, 16 and 4 pieces a workgroup"""
    rng = np.random.default_rng(n_seqs)
    seqs = [cases.random_adapter(rng, 20) for _ in range(n_seqs)]
    reads = [b"", cases.random_seq(rng, 19)]
    for pick in sorted({0, n_seqs - 1, n_seqs // 2}):
        reads.append(cases.random_seq(rng, S - 7) + seqs[pick] + cases.random_seq(rng, 300) + model.revcomp(seqs[n_seqs - 1 - pick]) + cases.random_seq(rng, 80))
        reads.append(cases.random_seq(rng, 2 * S - 20) + cases.substitute(rng, seqs[pick], 2) + cases.random_seq(rng, S + 3))
    want = check(ctx, seqs, 20, 40, 10, reads)
    assert all(len(w[3]) >= 2 for w in want[2:])


def test_ends_rule(ctx):
    """a mark partly inside the head cut, a mark reaching past e, end hits without middle hits and the reverse, all adapter"""
    rng = np.random.default_rng(7)
    seqs = [cases.LIGATION, cases.random_adapter(rng, 16)]
    reads = cases.end_rule_reads(rng, seqs) + [cases.random_seq(rng, 900), b"", b"N" * 30]
    want = check(ctx, seqs, 20, 60, 10, reads)
    assert (want[7][4], want[7][5], want[7][3]) == (-1, -1, [])
    assert want[6][0] == 0 and want[6][1] == 0 and len(want[6][3]) == 2
    assert (want[11][4], want[11][5], want[11][3]) == (0, 900, [])


@pytest.fixture(scope="module")
def mixed():
    rng = np.random.default_rng(21)
    seqs = [cases.LIGATION, cases.random_adapter(rng, 16)]
    reads = cases.end_rule_reads(rng, seqs) + cases.placements(rng, seqs, 10)[:12] + [cases.random_seq(rng, 5000), b"", cases.random_seq(rng, 60)]
    return seqs, reads, wanted(seqs, 20, 60, 10, reads)


@pytest.mark.parametrize("how", ["descending", "random"])
def test_orders(ctx, mixed, how):
    seqs, reads, want = mixed
    lengths = np.array([len(r) for r in reads])
    order = np.argsort(lengths, kind="stable").astype(np.uint32)[::-1].copy()
    if how == "random":
        order = np.random.default_rng(2).permutation(len(reads)).astype(np.uint32)
    ad = api.Adapters(seqs, errors=20, window=60, split_errors=10)
    check_marks(ctx, ad, seqs, reads, want, order=order)
    check_children(ctx, ad, seqs, reads, want, order=order)
    plane, offsets, lens = cases.pack(reads)
    for broken in (np.zeros(len(reads), dtype=np.uint32), np.arange(1, len(reads) + 1, dtype=np.uint32)):
        with pytest.raises(api.FlxError) as e:
            ctx.adapter_marks(plane, offsets, lens, ad, order=broken)
        assert e.value.code == 1
    with pytest.raises(api.FlxError):  # a read that leaves the plane
        ctx.adapter_marks(plane, offsets, np.where(np.arange(len(reads)) == len(reads) - 1, lens + 64, lens), ad)
    with pytest.raises(api.FlxError):  # an offset off the 16-byte grid
        ctx.adapter_marks(plane, offsets + np.uint64(1), lens, ad)
    ad.close()


def test_child_scores_and_capacity(ctx, mixed):
    """a parent keeps its own scores; a child gets the bits flx_score_batch gives its quality substring; FLX_ERR_CAPACITY"""
    seqs, reads, want = mixed
    quals = quals_of(reads)
    ad = api.Adapters(seqs, errors=20, window=60, split_errors=10)
    params = api.make_params(window_size=50, min_length=200, min_mean_q=5.0)
    got = check_children(ctx, ad, seqs, reads, want, params=params, child_capacity=1)  # (grows through FLX_ERR_CAPACITY)
    qplane, offsets, lengths = cases.pack(quals)
    plain = ctx.score_reads(qplane, offsets, lengths, params)
    assert (got["mean_q"].view(np.uint64) == plain["mean_q"].view(np.uint64)).all()
    assert (got["window_q"].view(np.uint64) == plain["window_q"].view(np.uint64)).all()
    gone = got["first"] == -1
    assert gone.any() and (got["passed"][gone] == 0).all() and (got["passed"][~gone] == plain["passed"][~gone]).all()
    subs = [quals[i][s:e] for i, w in enumerate(want) for s, e in w[3]]
    cplane, coffs, clens = cases.pack(subs)
    alone = ctx.score_reads(cplane, coffs, clens, params)
    assert (got["child_mean_q"].view(np.uint64) == alone["mean_q"].view(np.uint64)).all()
    assert (got["child_window_q"].view(np.uint64) == alone["window_q"].view(np.uint64)).all()
    assert (got["child_passed"] == alone["passed"]).all() and 0 < alone["passed"].sum() < len(subs)

    needed, n = len(subs), len(reads)
    splane, _, _ = cases.pack(reads, fill=seqs[0])
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
    ad.close()


def test_split_off_is_todays(ctx, mixed):
    """an object with the middle search off (never on, or turned off again) gives the children of the ends rule alone"""
    seqs, reads, _ = mixed
    pats = model.patterns(seqs)
    keys = model.keys_of(reads, 60, pats, 20)
    splane, offsets, lengths = cases.pack(reads, fill=seqs[0])
    qplane, _, _ = cases.pack(quals_of(reads))
    params = api.make_params(window_size=50)
    ad = api.Adapters(seqs, errors=20, window=60)
    for turn in range(2):
        assert ad.split_errors is None and ctx.L.flx_adapters_split(ad.h) == -1
        got = ctx.score_reads(qplane, offsets, lengths, params, adapters=ad, seq_plane=splane)
        children, coff = [], [0]
        for i, r in enumerate(reads):
            ch, first, last = model.child_of(len(r), keys[i, 0], keys[i, 1])
            assert (got["first"][i], got["last"][i]) == (first, last)
            children += ch
            coff.append(len(children))
        assert got["child_offsets"].tolist() == coff and got["child_ranges"].tolist() == [list(c) for c in children]
        with pytest.raises(api.FlxError) as e:
            ctx.adapter_marks(splane, offsets, lengths, ad)
        assert e.value.code == 1
        ad.set_split(10)
        assert ctx.L.flx_adapters_split(ad.h) == 10
        assert ctx.score_reads(qplane, offsets, lengths, params, adapters=ad, seq_plane=splane)["child_offsets"][-1] > len(children)
        ad.set_split(None)
    for bad in (41, -2):
        with pytest.raises(api.FlxError):
            ad.set_split(bad)
    assert (ctx.adapter_cuts(splane, offsets, lengths, ad) == keys).all()
    ad.close()
