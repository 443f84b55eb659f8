"""flx_phred_children with --trim_adapters as the producer, and flx_reads2_gather behind it, at the LAUNCH GEOMETRY the adapters tests
never reach (their largest child count is about 200).  One exact adapter at the head (E = 0, W = its length) makes every child's
length a chosen number; the batches come from tests/_geometry_cases.py and tests/test_geometry_cases.py proves on a CPU that they
are what is said here.  Held for equality against tests/_adapters_model.py (child_of), the call without adapters (parents), the
oracle's score_read and flx_score_batch over the children's quality substrings (bit for bit), and a plain loop (reads2).

What each batch is the first test to execute, with --trim_adapters as producer:

  child counts 1, 2                       flx_radix_sort_pairs (csrc/sort.hip) returns at `n <= 1`; the smallest sort
  1023, 1024, 1025  (RS_TILE +- 1)        k_radix_hist / k_radix_scatter with a last wave tile that is one short, full, and a second
                                          tile of one key (`i < n` per round; tiles = 2)
  4095, 4096, 4097  (RS_TILE * RS_WAVES)  the same for the workgroup: `tile < n_tiles` fails for waves of the last block; a second
                                          block for one key.  1024 and 4096 children: k_qsplit_child_slots (csrc/qsplit.hip) launches
                                          (nc + 1 + 255) / 256 blocks and the sentinel slot[nc] sits alone in the last
  all children one length                 no key bit varies: every pass is skipped (`continue`), the order is vals0 as written
  lengths within 1 .. 255                 exactly one pass: the sorted order is in the SECOND buffer (keys1 / vals1)
  lengths 1 .. 60 000                     two passes: back in the first buffer; k_scan_apply over a child plane of megabytes
  a few children of 1024 bases and more   the 128-byte child slots (`cl >= 1024 ? 112 : 0`, k_qsplit_child_starts) among 16-byte
                                          ones: gaps in the child plane
  255, 256, 257, 511, 512, 2047, 2048     reads, with children from none, some and all of them, the last read among them:
                                          k_adapter_children and k_reads2_sizes launch (n + 1 + 255) / 256 blocks, for n % 256 == 0 the
                                          sentinel n_child[n] / sizes[n] is alone in its block; n + 1 = SCAN_TILE and SCAN_TILE + 1
                                          entries through flx_exclusive_scan_i64: the sentinel as the last entry of a full tile and
                                          alone in a second; k_adapter_emit's `child_offsets[r + 1]` of the last read

Sequence planes are filled with the adapter's own sequence between the reads; the host-array forms prefill their outputs with 0xA5."""
import numpy as np
import pytest

import _adapters_cases as cases
import _adapters_model as model
import _geometry_cases as geo
from filtlong_amd import api

pytestmark = pytest.mark.gpu
PARAMS = dict(window_size=50, min_length=64, min_mean_q=90.0)


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ad():
    a = api.Adapters([geo.CHILD_ADAPTER], errors=geo.CHILD_E, window=geo.CHILD_W)
    yield a
    a.close()


@pytest.fixture(scope="module")
def text_cache():
    return {}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def check(ctx, ad, oracle, text_cache, reads, quals, order_too=True):
    """one batch through flx_score_batch_adapters and flx_reads2_gather; returns the scores"""
    n = len(reads)
    keys, kids = geo.children_of(reads, text_cache)
    nc = len(kids)
    splane, offsets, lengths = cases.pack(reads, fill=geo.CHILD_ADAPTER)
    qplane, qoff, _ = cases.pack(quals)
    assert (qoff == offsets).all()
    params = api.make_params(**PARAMS)
    plain = ctx.score_reads(qplane, offsets, lengths, params)
    subs = [quals[p][s:e] for p, s, e in kids]
    alone = None
    if nc:  # a child gets the bits flx_score_batch gives its quality substring
        cplane, coffs, clens = cases.pack(subs)
        alone = ctx.score_reads(cplane, coffs, clens, params)
    coff = np.zeros(n + 1, dtype=np.uint64)
    for p, _, _ in kids:
        coff[p + 1] += 1
    coff = np.cumsum(coff).astype(np.uint64)
    firsts = np.array([model.child_of(len(r), k[0], k[1])[1:] for r, k in zip(reads, keys)], dtype=np.int32).reshape(-1, 2)
    got = None
    for order in ((None, api.length_order(lengths)) if order_too else (None,)):
        got = ctx.score_reads(qplane, offsets, lengths, params, order=order, adapters=ad, seq_plane=splane, child_capacity=max(nc, 1))
        assert (got["first"] == firsts[:, 0]).all() and (got["last"] == firsts[:, 1]).all()
        assert (got["child_offsets"] == coff).all()
        assert got["child_ranges"].tolist() == [[s, e] for _, s, e in kids]
        # a parent keeps its own scores; one with nothing left fails
        assert (bits(got["mean_q"]) == bits(plain["mean_q"])).all() and (bits(got["window_q"]) == bits(plain["window_q"])).all()
        gone = got["first"] == -1
        assert (got["passed"][gone] == 0).all() and (got["passed"][~gone] == plain["passed"][~gone]).all()
        assert len(got["child_mean_q"]) == nc
        if nc:
            assert (bits(got["child_mean_q"]) == bits(alone["mean_q"])).all()
            assert (bits(got["child_window_q"]) == bits(alone["window_q"])).all()
            assert (got["child_passed"] == alone["passed"]).all()
    if nc:  # the oracle on the first, the last and 200 random children
        op = oracle.make_params(**PARAMS)
        pick = sorted({0, nc - 1} | set(np.random.default_rng(nc).choice(nc, size=min(nc, 200), replace=False).tolist()))
        for c in pick:
            w = oracle.score_read(None, subs[c], op)
            assert bits([w["mean_q"]])[0] == bits(got["child_mean_q"])[c] and bits([w["window_q"]])[0] == bits(got["child_window_q"])[c], c
            assert w["passed"] == got["child_passed"][c], c
        if nc >= 100:
            assert 0 < int(got["child_passed"].sum()) < nc
    check_reads2(ctx, lengths, got)
    check_reads2(ctx, lengths, plain)
    return got


def check_reads2(ctx, lengths, sc):
    """the reference's rule: a read without children in its place, else its children in its place"""
    rows = []
    coff = sc["child_offsets"].tolist()
    mq, wq, ps = bits(sc["mean_q"]).tolist(), bits(sc["window_q"]).tolist(), sc["passed"].tolist()
    cmq, cwq, cps = bits(sc["child_mean_q"]).tolist(), bits(sc["child_window_q"]).tolist(), sc["child_passed"].tolist()
    clen = (sc["child_ranges"][:, 1] - sc["child_ranges"][:, 0]).tolist()
    for i in range(len(lengths)):
        c0, c1 = coff[i], coff[i + 1]
        if c0 == c1:
            rows.append((mq[i], wq[i], int(lengths[i]), ps[i], i, -1))
        for k in range(c0, c1):
            rows.append((cmq[k], cwq[k], clen[k], cps[k], i, k))
    r2 = ctx.reads2_gather(lengths, sc)
    got = list(zip(bits(r2["mean_q"]).tolist(), bits(r2["window_q"]).tolist(), r2["length"].tolist(), r2["passed"].tolist(),
                   r2["parent"].tolist(), r2["child"].tolist()))
    assert len(got) == len(rows)
    bad = [i for i, (g, w) in enumerate(zip(got, rows)) if g != w]
    assert not bad, [(i, got[i], rows[i]) for i in bad[:5]]


@pytest.mark.parametrize("nc,cls", geo.CHILD_BATCHES)
def test_child_counts_and_length_classes(ctx, ad, oracle, text_cache, nc, cls):
    reads, quals, designed = geo.children_batch(nc, cls)
    got = check(ctx, ad, oracle, text_cache, reads, quals)
    lens = got["child_ranges"][:, 1] - got["child_ranges"][:, 0]
    assert len(lens) == nc and (lens == designed[designed > 0]).all()
    assert geo.sort_passes(lens) == geo.SORT_PASSES[cls]


@pytest.mark.parametrize("n_reads,share", geo.READ_BATCHES)
def test_read_counts(ctx, ad, oracle, text_cache, n_reads, share):
    reads, quals, designed = geo.reads_batch(n_reads, share)
    got = check(ctx, ad, oracle, text_cache, reads, quals)
    assert len(got["child_mean_q"]) == int((designed > 0).sum())
    assert (int(got["child_offsets"][-1]) > int(got["child_offsets"][-2])) == (share != "none")  # the last read's child


def test_one_context_shrinking_and_growing(ctx, ad, oracle, text_cache):
    """the largest batch, one read, reads without a child, the largest again: workspaces 0 to 2 and the scratch are reused, and no
    count or sentinel of the larger call may be left in the smaller"""
    nc, cls = max(geo.CHILD_BATCHES, key=lambda b: (b[0], b[1] == "wide"))
    assert (nc, cls) == (geo.RS_BLOCK + 1, "wide")
    reads, quals, _ = geo.children_batch(nc, cls)
    first = check(ctx, ad, oracle, text_cache, reads, quals, order_too=False)
    one, one_q, _ = geo.children_batch(1, "one")
    at = next(i for i, r in enumerate(one) if len(r) > geo.CHILD_W)
    got = check(ctx, ad, oracle, text_cache, one[at:at + 1], one_q[at:at + 1], order_too=False)
    assert len(got["child_mean_q"]) == 1
    quiet, quiet_q, _ = geo.reads_batch(257, "none")
    got = check(ctx, ad, oracle, text_cache, quiet, quiet_q, order_too=False)
    assert len(got["child_mean_q"]) == 0 and int(got["child_offsets"][-1]) == 0
    again = check(ctx, ad, oracle, text_cache, reads, quals, order_too=False)
    for k in first:
        a, b = np.asarray(first[k]), np.asarray(again[k])
        assert a.shape == b.shape and (bits(a) == bits(b) if a.dtype == np.float64 else a == b).all(), k
