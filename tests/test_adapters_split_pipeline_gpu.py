"""A Phred-mode pipeline whose adapters have the middle search on: whatever the chunk size, and with growing slots, the children are
the model's (tests/_adapters_split_model.py) and every value is what ONE flx_score_batch_adapters call gives for all reads; the keys
stay those of the ends rule; with a screen as well, the reads the screen's MODEL excludes fail together with all their children."""
import numpy as np
import pytest

import _adapters_cases as cases
import _adapters_model as model
import _adapters_split_model as split
import _screen_model as smodel
from filtlong_amd import api, synth

pytestmark = pytest.mark.gpu
WINDOW, ERRORS, SPLIT_ERRORS, PERCENT = 80, 20, 10, 10.0
SAME = ("mean_q", "window_q", "passed", "first", "last", "child_offsets", "child_ranges", "child_mean_q", "child_window_q", "child_passed")


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def world(ctx):
    """reads of 100 to 4000 bases: half of them chimeras of two or three parts, some with adapters at the ends too; a contaminant X"""
    rng = np.random.default_rng(199)
    seqs = [cases.LIGATION, cases.random_adapter(rng, 20)]
    xref = smodel.random_seq(rng, 4000)
    reads = []
    for i in range(60):
        part = lambda: smodel.draw(rng, xref, int(rng.integers(400, 1500)), 0.03) if i % 4 == 0 else cases.random_seq(rng, int(rng.integers(100, 2000)))
        r = part()
        if i % 2 == 0:
            r += cases.substitute(rng, seqs[i % 4 // 2], 1) + part()
        if i % 10 == 4:
            r += model.revcomp(seqs[1]) + part()
        if i % 5 == 1:
            r = seqs[0] + r
        if i % 5 == 2:
            r += model.revcomp(seqs[1]) + cases.random_seq(rng, 4)
        reads.append(r)
    reads += [b"", b"ACGT", cases.LIGATION * 3, cases.random_seq(rng, 79), cases.random_seq(rng, 1030)]
    quals = [synth.qual_read(700 + i, len(r)).tobytes() if len(r) else b"" for i, r in enumerate(reads)]
    pats = model.patterns(seqs)
    want = [split.split_of(r, WINDOW, pats, ERRORS, SPLIT_ERRORS) for r in reads]
    xs = api.Kmers(ctx)
    xs.add_screen_fasta([xref])
    xs.finalize()
    x = smodel.build_set([xref])
    hits = np.array([smodel.hits(x, s) for s in reads], dtype=np.uint32)
    excl = np.array([smodel.excluded(h, len(s), PERCENT) for h, s in zip(hits, reads)], dtype=np.uint8)
    ad = api.Adapters(seqs, errors=ERRORS, window=WINDOW, split_errors=SPLIT_ERRORS)
    params = api.make_params(window_size=100, min_length=300, min_mean_q=5.0)
    splane, offsets, lengths = cases.pack(reads)
    qplane, _, _ = cases.pack(quals)
    one = ctx.score_reads(qplane, offsets, lengths, params, adapters=ad, seq_plane=splane)
    yield {"reads": reads, "quals": quals, "want": want, "xs": xs, "hits": hits, "excl": excl, "ad": ad, "params": params, "one": one}
    xs.close()
    ad.close()


def chunked(items, size):
    return [items[i:i + size] for i in range(0, len(items), size)]


def pairs(w, size):
    return list(zip(chunked(w["quals"], size), chunked(w["reads"], size)))


def test_one_call_is_the_model(world):
    w = world
    children, coff = [], [0]
    for i, x in enumerate(w["want"]):
        assert (w["one"]["first"][i], w["one"]["last"][i]) == (x[4], x[5]), i
        children += x[3]
        coff.append(len(children))
    assert w["one"]["child_offsets"].tolist() == coff and w["one"]["child_ranges"].tolist() == [list(c) for c in children]
    per = np.diff(np.array(coff))
    assert (per == 2).sum() >= 15 and (per == 3).sum() >= 3 and (per == 0).sum() >= 10 and (w["one"]["first"] == -1).sum() >= 1


@pytest.mark.parametrize("size,grow", [(3, False), (25, True)])
def test_chunks_and_growing_slots(ctx, world, size, grow):
    w = world
    kw = dict(chunk_bytes=4096 if grow else 1 << 16, chunk_reads=4 if grow else 64, grow=grow)
    got = ctx.score_stream(pairs(w, size), w["params"], adapters=w["ad"], **kw)
    keys = np.array([[x[0], x[1]] for x in w["want"]], dtype=np.uint32)
    assert (got["adapter_keys"] == keys).all()
    for k in SAME:
        assert got[k].tobytes() == w["one"][k].tobytes(), k
    assert 0 < got["child_passed"].sum() < len(got["child_passed"])


def test_with_a_screen(ctx, world):
    """one sequence plane serves both; the screen looks at the whole parent, and an excluded parent's children all fail"""
    w = world
    got = ctx.score_stream(pairs(w, 9), w["params"], chunk_bytes=1 << 16, chunk_reads=16, adapters=w["ad"], exclude=w["xs"], exclude_percent=PERCENT)
    assert (got["hits"] == w["hits"]).all() and (got["excluded"] == w["excl"]).all()
    want = {k: v.copy() for k, v in w["one"].items()}
    want["passed"][w["excl"] != 0] = 0
    with_children = 0
    for i in np.flatnonzero(w["excl"]):
        a, b = int(want["child_offsets"][i]), int(want["child_offsets"][i + 1])
        with_children += int(b - a >= 2 and want["child_passed"][a:b].sum() > 0)
        want["child_passed"][a:b] = 0
    assert with_children >= 3, "excluded parents with two children or more, some of which had passed"
    for k in SAME:
        assert got[k].tobytes() == want[k].tobytes(), k
