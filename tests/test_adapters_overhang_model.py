"""The definition of --adapter_overhang on tests/_adapters_overhang_model.py alone (no GPU, no library): what follows from the rule
whatever computes it, and that the model at O = 0 is the model of --trim_adapters."""
import numpy as np
import pytest

import _adapters_cases as cases
import _adapters_model as plain
import _adapters_overhang_cases as ocases
import _adapters_overhang_model as model


def test_allowances():
    """O_p = min(O, m - 12), k'_p = (m - O_p) * E / 100"""
    want = {  # (m, O): O_p
        (12, 0): 0, (12, 1): 0, (12, 16): 0, (12, 52): 0, (13, 0): 0, (13, 1): 1, (13, 16): 1, (13, 52): 1,
        (28, 0): 0, (28, 1): 1, (28, 16): 16, (28, 52): 16, (64, 0): 0, (64, 1): 1, (64, 16): 16, (64, 52): 52,
    }
    for (m, o), o_p in want.items():
        assert model.overhang_of(m, o) == o_p
        for errors in (0, 20, 40):
            assert model.edits_anchored(m, errors, o) == (m - o_p) * errors // 100
    assert model.edits_anchored(28, 20, 8) == 4 and model.edits_anchored(28, 20, 16) == 2 and model.edits_anchored(64, 40, 1) == 25
    assert model.MAX_OVERHANG == 52
    assert max(m + model.edits_anchored(m, e, o) for m in range(12, 65) for e in range(41) for o in range(1, 53) if model.overhang_of(m, o)) == 89  # the longest anchored walk: m = 64, O = 1, E = 40


def test_overhang_zero_is_the_plain_rule():
    rng = np.random.default_rng(3)
    seqs = [cases.LIGATION, cases.random_adapter(rng, 12), cases.random_adapter(rng, 33)]
    pats = model.patterns(seqs)
    reads = cases.reads_for(rng, seqs, 40)
    assert (model.keys_of(reads, 40, pats, 20, 0) == plain.keys_of(reads, 40, pats, 20)).all()


@pytest.mark.parametrize("overhang,errors,window", [(8, 20, 150), (52, 40, 60), (1, 0, 30)])
def test_the_key_only_grows(overhang, errors, window):
    """per read end the key with O is >= the key without it, on random and planted reads"""
    rng = np.random.default_rng(overhang)
    seqs = [cases.LIGATION, cases.random_adapter(rng, 13), cases.random_adapter(rng, 64)]
    pats = model.patterns(seqs)
    reads = ocases.reads_for(rng, seqs, errors, window, overhang, planted=1) + [cases.random_seq(rng, int(n)) for n in rng.integers(0, 400, size=30)]
    with_o, without = model.keys_of(reads, window, pats, errors, overhang), model.keys_of(reads, window, pats, errors, 0)
    assert (with_o >= without).all()
    if window >= 40 and errors <= 20:  # (at E = 40 the free walk finds nearly every remnant itself)
        assert (with_o > without).sum() > 10 and ((with_o == without) & (without > 0)).any()


@pytest.mark.parametrize("m,overhang,errors", [(28, 8, 20), (28, 16, 20), (13, 5, 20), (64, 52, 40), (40, 11, 0)])
def test_exact_remnants(m, overhang, errors):
    """pattern[x:] + random hits by overhang for x <= O_p; for x = O_p + k'_p + 1 only if the free walk hits"""
    rng = np.random.default_rng(m + overhang)
    a = cases.LIGATION if m == 28 else cases.random_adapter(rng, m)
    pats = model.patterns([a])
    o, k = model.overhang_of(m, overhang), model.edits_anchored(m, errors, overhang)
    for x in range(0, o + 1):
        for side, read in ((0, a[x:] + cases.random_seq(rng, 300)), (1, cases.random_seq(rng, 300) + model.revcomp(a)[:m - x])):
            free, anchored = model.end_walks(read, side, 150, pats, errors, overhang)[1 if side else 0]
            assert anchored is not None and anchored[0] == 0 and anchored[1] >= m - x, (x, side)
            assert model.end_key(read, side, 150, pats, errors, overhang) >> 8 >= m - x
    x = o + k + 1
    if x < m:
        # The remnant pays x - O_p = k' + 1 edits where it ends.  (A cheaper alignment needs the bases behind it to continue the
        # pattern; the tail here is the complement of what the pattern would want, base by base, so none does.)
        other = bytes.maketrans(b"ACGT", b"CATG")
        read = a[x:] + (a * 12).translate(other)[m - x:m - x + 300]
        free, anchored = model.end_walks(read, 0, 150, pats, errors, overhang)[0]
        assert int(model.last_rows([a], read[:150], o)[0][m - x - 1]) == k + 1
        assert anchored is None or free is not None


def test_truncation_beyond_the_allowance_needs_the_free_walk():
    """x = O_p + k'_p + 1 with a tail that shares nothing with the pattern: the anchored walk pays k' + 1 and does not hit"""
    a = b"ACGTTGCAACGGTTCAGCATCGATTGCA"  # 28 bases
    m, overhang, errors = 28, 8, 20
    o, k = model.overhang_of(m, overhang), model.edits_anchored(m, errors, overhang)
    assert (o, k) == (8, 4)
    for x in (o + k + 1, o + k + 2):
        read = a[x:] + b"N" * 200
        free, anchored = model.end_walks(read, 0, 150, model.patterns([a]), errors, overhang)[0]
        assert free is None and anchored is None
        assert int(model.last_rows([a], read[:150], o)[0].min()) == x - o
        assert model.end_key(read, 0, 150, model.patterns([a]), errors, overhang) == 0
    read = a[o + k:] + b"N" * 200  # the last truncation the allowance pays for
    assert model.end_walks(read, 0, 150, model.patterns([a]), errors, overhang)[0] == (None, (k, m - o - k))
    assert model.end_key(read, 0, 150, model.patterns([a]), errors, overhang) == ((m - o - k) << 8)
    # at the tail the END of the adapter is the missing part
    read = b"N" * 200 + a[:m - o]
    assert model.end_walks(read, 1, 150, model.patterns([a]), errors, overhang)[0] == (None, (0, m - o))


def test_both_walks_different_j():
    a = cases.LIGATION
    pats = model.patterns([a])
    read = a[8:] + b"CCC" + a + b"G" * 100
    free, anchored = model.end_walks(read, 0, 150, pats, 20, 8)[0]
    assert anchored == (0, 20) and free == (0, 51)
    assert model.end_key(read, 0, 150, pats, 20, 8) == 51 << 8
    assert model.end_key(a[8:] + b"G" * 100, 0, 150, pats, 20, 8) == 20 << 8 and model.end_key(a[8:] + b"G" * 100, 0, 150, pats, 20, 0) == 0


def test_anchoring():
    """the remnant two bases behind the edge: the free walk of the whole pattern does not see it, the anchored walk pays for the two"""
    a = cases.LIGATION
    pats = model.patterns([a])
    read = b"GG" + a[8:] + b"G" * 100
    assert model.end_walks(read, 0, 150, pats, 20, 8)[0] == (None, (2, 22))
    read = b"G" * 6 + a[8:] + b"G" * 100
    assert model.end_walks(read, 0, 150, pats, 20, 8)[0] == (None, None)
