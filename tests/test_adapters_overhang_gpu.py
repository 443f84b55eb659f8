"""flx_adapter_cuts of an object with an overhang (flx_adapters_set_overhang) against tests/_adapters_overhang_model.py, for equality.

The shapes are the smallest at which the second walk can go wrong: patterns of 12 (no second walk), 13, 32, 63 and 64 bases (bit 63
of the first column ~0 << O_p, the top bit at m = 64) in ONE set; O of 1, 11, 12, 51 and 52; E of 0, 20 and 40; W of 1, 12, 150 and
1024; read lengths on every edge of the walk (0, 1, m - O_p - 1, m - O_p, m - O_p + k', m + k', m + k' + 1, W - 1, W, W + 1);
truncations O_p - 1, O_p and O_p + 1 at the head and, with the adapter's end cut off, at the tail (tests/_adapters_overhang_cases.py).

Planes are filled with the adapter's own sequence between the reads, and every call goes through the host-array form, which prefills
the device keys with 0xA5 (test_adapters_gpu.py)."""
import numpy as np
import pytest

import _adapters_cases as cases
import _adapters_overhang_cases as ocases
import _adapters_overhang_model as model
from filtlong_amd import api

pytestmark = pytest.mark.gpu

EDGE_M = (13, 32, 63, 64, 12)


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


def same(got, want, reads):
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, [(int(i), len(reads[i]), got[i].tolist(), want[i].tolist()) for i in bad[:8]]


def cuts(ctx, ad, seqs, reads, order=None):
    plane, offsets, lengths = cases.pack(reads, fill=bytes(seqs[0]).upper())
    return ctx.adapter_cuts(plane, offsets, lengths, ad, order=order)


def edge_seqs(seed, first):
    """one sequence of every length of EDGE_M, the one of `first` bases in front (the reads are planted with the first ones)"""
    rng = np.random.default_rng(seed)
    seqs = {m: cases.random_adapter(rng, m) for m in EDGE_M}
    return [seqs[first]] + [seqs[m] for m in EDGE_M if m != first]


# (O, E, W, the pattern length planted first): every O, E, W and m of the lists above at least once, the extremes together
CONFIGS = [(1, 40, 150, 64), (11, 20, 150, 32), (12, 0, 150, 63), (51, 20, 150, 64), (52, 40, 150, 63), (52, 0, 1024, 64), (1, 20, 1024, 13),
           (11, 40, 12, 13), (12, 20, 12, 32), (52, 20, 1, 64), (8, 20, 150, 13)]


@pytest.mark.parametrize("overhang,errors,window,first", CONFIGS)
def test_edges(ctx, overhang, errors, window, first):
    seqs = edge_seqs(overhang + window, first)
    rng = np.random.default_rng(1000 * overhang + errors + window)
    reads = ocases.reads_for(rng, seqs, errors, window, overhang, planted=1 if window > 150 else 2)
    pats = model.patterns(seqs)
    want, plain = model.keys_of(reads, window, pats, errors, overhang, with_plain=True)
    ad = api.Adapters(seqs, errors=errors, window=window, overhang=overhang)
    assert ad.overhang == overhang and len(ad) == len(pats)
    same(cuts(ctx, ad, seqs, reads), want, reads)
    lengths = np.array([len(r) for r in reads], dtype=np.int32)
    for order in (api.length_order(lengths), np.random.default_rng(3).permutation(len(reads)).astype(np.uint32)):
        same(cuts(ctx, ad, seqs, reads, order=order), want, reads)
    ad.close()
    assert (want >= plain).all()
    if window >= 150 and errors <= 20 and overhang >= 8:
        assert (want > plain).sum() >= 3  # the overhang decides somewhere


def test_both_walks_hit_at_different_j(ctx):
    a = cases.LIGATION
    reads = [a[8:] + b"CCC" + a + b"G" * 200, a[8:] + b"G" * 200, b"G" * 200 + model.revcomp(a) + b"CC" + a[:20], b"G" * 200 + a[:20]]
    pats = model.patterns([a])
    want = model.keys_of(reads, 150, pats, 20, 8)
    assert want.tolist() == [[51 << 8, 0], [20 << 8, 0], [0, (50 << 8) | 1], [0, 20 << 8]]
    ad = api.Adapters([a], errors=20, window=150, overhang=8)
    same(cuts(ctx, ad, [a], reads), want, reads)
    ad.close()


def test_n_and_lower_case_inside_the_remnant(ctx):
    rng = np.random.default_rng(12)
    a = cases.LIGATION
    rem = ocases.with_n_and_lower(a[6:])
    reads = [rem + cases.random_seq(rng, 300), cases.random_seq(rng, 300) + ocases.with_n_and_lower(a[:22]), (a[8:] + cases.random_seq(rng, 200)).lower(),
             b"N" * 20 + cases.random_seq(rng, 200), a[8:18] + b"NNNNN" + a[23:] + cases.random_seq(rng, 200)]
    want = model.keys_of(reads, 150, model.patterns([a]), 20, 8)
    assert want[0, 0] >> 8 == 22 and want[1, 1] >> 8 == 22 and want[2, 0] >> 8 == 20 and want[3].tolist() == [0, 0] and want[4, 0] == 0
    ad = api.Adapters([a], errors=20, window=150, overhang=8)
    same(cuts(ctx, ad, [a], reads), want, reads)
    ad.close()


def test_a_twelve_base_pattern_has_no_second_walk(ctx):
    """a set mixing m = 12 (O_p = 0) with longer patterns: the 12-mer's remnant is found by no walk, the 28-mer's is"""
    rng = np.random.default_rng(5)
    short, a = b"GATTACAGGCTC", cases.LIGATION
    seqs = [short, a]
    reads = [short[2:] + b"N" * 200, a[8:] + b"N" * 200, short + b"N" * 200, b"N" * 200 + short[:10], b"N" * 200 + a[:20], cases.random_seq(rng, 200)]
    want = model.keys_of(reads, 150, model.patterns(seqs), 0, 16)
    assert want.tolist() == [[0, 0], [(20 << 8) | 2, 0], [12 << 8, 0], [0, 0], [0, (20 << 8) | 2], [0, 0]]
    ad = api.Adapters(seqs, errors=0, window=150, overhang=16)
    same(cuts(ctx, ad, seqs, reads), want, reads)
    ad.close()


def test_set_overhang_after_a_first_call(ctx):
    """the device holds the table of the first call: a change must reach it; back to 0 gives the keys of a fresh object"""
    rng = np.random.default_rng(77)
    seqs = [cases.LIGATION, cases.random_adapter(rng, 40)]
    reads = ocases.reads_for(rng, seqs, 20, 150, 8, planted=2)
    pats = model.patterns(seqs)
    want = {o: model.keys_of(reads, 150, pats, 20, o) for o in (0, 8, 16)}
    assert (want[8] != want[0]).any() and (want[16] != want[8]).any()
    ad = api.Adapters(seqs, errors=20, window=150)
    assert ad.overhang == 0
    same(cuts(ctx, ad, seqs, reads), want[0], reads)
    for o in (8, 16, 8, 0, 16):
        ad.overhang = o
        assert ad.overhang == o
        same(cuts(ctx, ad, seqs, reads), want[o], reads)
    ad.overhang = 0
    fresh = api.Adapters(seqs, errors=20, window=150)
    got = cuts(ctx, ad, seqs, reads)
    same(got, cuts(ctx, fresh, seqs, reads), reads)
    same(got, want[0], reads)
    for bad in (-1, 53, 1000):
        with pytest.raises(api.FlxError) as e:
            ad.overhang = bad
        assert e.value.code == 1 and ad.overhang == 0
    with pytest.raises(api.FlxError):
        api.Adapters(seqs, errors=20, window=150, overhang=53)
    ad.close()
    fresh.close()
