"""An object with an overhang behind the keys: flx_score_batch_adapters and a Phred-mode pipeline follow it.  The children are the
model's (tests/_adapters_overhang_model.py for the keys, the child rule of tests/_adapters_model.py), a child cut by an overhang hit
gets the bits flx_score_batch gives its quality substring, a pipeline over several chunks gives what ONE call gives, and with
split_errors set the middle search (tests/_adapters_split_model.py) starts from the [s, e) the overhang keys leave."""
import numpy as np
import pytest

import _adapters_cases as cases
import _adapters_overhang_model as model
import _adapters_split_model as split
from filtlong_amd import api, synth

pytestmark = pytest.mark.gpu
WINDOW, ERRORS, OVERHANG, SPLIT_ERRORS = 80, 20, 8, 10
SAME = ("mean_q", "window_q", "passed", "first", "last", "child_offsets", "child_ranges", "child_mean_q", "child_window_q", "child_passed")


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def world():
    """reads of 300 to 2500 bases: remnants of 20 to 22 adapter bases at the head, at the tail, at both, whole adapters, chimeras"""
    rng = np.random.default_rng(811)
    seqs = [cases.LIGATION, cases.random_adapter(rng, 24)]
    reads = []
    for i in range(50):
        a = seqs[i % 2]
        x = 6 + i % 3
        r = cases.random_seq(rng, int(rng.integers(300, 2500)))
        if i % 10 == 7:
            r += a + cases.random_seq(rng, int(rng.integers(300, 900)))  # an adapter inside: the middle search's
        if i % 4 in (0, 1):
            r = a[x:] + r
        if i % 4 in (1, 2):
            r = r + model.revcomp(a)[:len(a) - x]
        if i % 12 == 3:
            r = cases.random_seq(rng, 3) + a + r
        reads.append(r)
    reads += [b"", b"ACGT", cases.LIGATION[8:], cases.LIGATION[8:] + model.revcomp(cases.LIGATION)[:20], cases.random_seq(rng, 1030)]
    quals = [synth.qual_read(900 + i, len(r)).tobytes() if len(r) else b"" for i, r in enumerate(reads)]
    pats = model.patterns(seqs)
    keys, plain = model.keys_of(reads, WINDOW, pats, ERRORS, OVERHANG, with_plain=True)
    assert (keys > plain).sum() >= 30 and ((keys == plain) & (plain > 0)).any()
    return {"seqs": seqs, "reads": reads, "quals": quals, "pats": pats, "keys": keys, "plain": plain,
            "params": api.make_params(window_size=100, min_length=400, min_mean_q=5.0)}


def chunked(items, size):
    return [items[i:i + size] for i in range(0, len(items), size)]


def check_children(ctx, w, got, want_children):
    """want_children: per read (children, first, last)"""
    children, parents, coff = [], [], [0]
    for i, (ch, first, last) in enumerate(want_children):
        assert (got["first"][i], got["last"][i]) == (first, last), i
        children += ch
        parents += [i] * len(ch)
        coff.append(len(children))
    assert got["child_offsets"].tolist() == coff and got["child_ranges"].tolist() == [list(c) for c in children]
    # a child gets the bits flx_score_batch gives its quality substring
    subs = [w["quals"][p][s:e] for p, (s, e) in zip(parents, children)]
    cplane, coffs, clens = cases.pack(subs)
    alone = ctx.score_reads(cplane, coffs, clens, w["params"])
    assert (got["child_mean_q"].view(np.uint64) == alone["mean_q"].view(np.uint64)).all()
    assert (got["child_window_q"].view(np.uint64) == alone["window_q"].view(np.uint64)).all()
    assert (got["child_passed"] == alone["passed"]).all() and 0 < alone["passed"].sum() < len(subs)
    return children, parents


def test_children_of_overhang_hits(ctx, world):
    w = world
    splane, offsets, lengths = cases.pack(w["reads"])
    qplane, _, _ = cases.pack(w["quals"])
    ad = api.Adapters(w["seqs"], errors=ERRORS, window=WINDOW, overhang=OVERHANG)
    one = ctx.score_reads(qplane, offsets, lengths, w["params"], adapters=ad, seq_plane=splane)
    want = [model.child_of(len(r), k[0], k[1]) for r, k in zip(w["reads"], w["keys"])]
    children, parents = check_children(ctx, w, one, want)
    by_overhang = [(w["keys"][p] > w["plain"][p]).any() for p in parents]
    assert sum(by_overhang) >= 25 and (one["first"] == -1).sum() >= 2
    ad.overhang = 0  # the same object without: other children
    off = ctx.score_reads(qplane, offsets, lengths, w["params"], adapters=ad, seq_plane=splane)
    check_children(ctx, w, off, [model.child_of(len(r), k[0], k[1]) for r, k in zip(w["reads"], w["plain"])])
    assert off["child_ranges"].tolist() != one["child_ranges"].tolist()
    ad.close()


@pytest.mark.parametrize("size,grow", [(3, False), (20, True)])
def test_chunks_against_one_call(ctx, world, size, grow):
    w = world
    splane, offsets, lengths = cases.pack(w["reads"])
    qplane, _, _ = cases.pack(w["quals"])
    ad = api.Adapters(w["seqs"], errors=ERRORS, window=WINDOW, overhang=OVERHANG)
    one = ctx.score_reads(qplane, offsets, lengths, w["params"], adapters=ad, seq_plane=splane)
    kw = dict(chunk_bytes=4096 if grow else 1 << 16, chunk_reads=4 if grow else 64, grow=grow)
    got = ctx.score_stream(list(zip(chunked(w["quals"], size), chunked(w["reads"], size))), w["params"], adapters=ad, **kw)
    assert (got["adapter_keys"] == w["keys"]).all()
    for k in SAME:
        assert got[k].tobytes() == one[k].tobytes(), k
    ad.close()


def test_the_middle_search_starts_from_the_new_range(ctx, world):
    w = world
    splane, offsets, lengths = cases.pack(w["reads"])
    qplane, _, _ = cases.pack(w["quals"])
    want = []
    for r, k in zip(w["reads"], w["keys"]):
        want.append(split.children(len(r), int(k[0]), int(k[1]), split.marks(r, w["pats"], SPLIT_ERRORS)))
    ad = api.Adapters(w["seqs"], errors=ERRORS, window=WINDOW, split_errors=SPLIT_ERRORS, overhang=OVERHANG)
    one = ctx.score_reads(qplane, offsets, lengths, w["params"], adapters=ad, seq_plane=splane)
    check_children(ctx, w, one, want)
    per = np.diff(one["child_offsets"].astype(np.int64))
    assert (per == 2).sum() >= 3 and (per == 1).sum() >= 20
    got = ctx.score_stream(list(zip(chunked(w["quals"], 7), chunked(w["reads"], 7))), w["params"], adapters=ad, chunk_bytes=1 << 16, chunk_reads=16)
    assert (got["adapter_keys"] == w["keys"]).all()
    for k in SAME:
        assert got[k].tobytes() == one[k].tobytes(), k
    ad.close()
