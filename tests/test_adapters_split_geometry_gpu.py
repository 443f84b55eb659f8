"""How csrc/adapters_split.hip cuts the work, on the GPU: batches whose piece count is one less than, exactly and one more than a
workgroup's share, at least three workgroups with a partial last one, a hit on both sides of every workgroup boundary, reads whose
pieces fall into different workgroups; 255, 256 and 257 reads (the sentinel of the child walk); 1, 1023, 1024 and 1025 children.
tests/test_adapters_split_cases.py checks, without a GPU, that the batches are what they are taken for.  Everything is compared
with tests/_adapters_split_model.py for equality."""
import numpy as np
import pytest

import _adapters_split_cases as cases
from _adapters_split_checks import check_children, check_marks, wanted
from filtlong_amd import api

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("kind", cases.PIECE_KINDS)
@pytest.mark.parametrize("n_seqs", cases.PIECE_SETS)
def test_piece_batches(ctx, n_seqs, kind):
    seqs, proc, counts, ppb = cases.piece_batch(n_seqs, kind)
    want_proc = wanted(seqs, 0, 1, 0, proc)
    ad = api.Adapters(seqs, errors=0, window=1, split_errors=0)
    check_marks(ctx, ad, seqs, proc, want_proc)
    check_children(ctx, ad, seqs, proc, want_proc)
    # the same batch with the reads somewhere else in the input: `order` is the processing order
    order = np.random.default_rng(n_seqs).permutation(len(proc)).astype(np.uint32)
    inp, want = [None] * len(proc), [None] * len(proc)
    for place, r in enumerate(order):
        inp[int(r)], want[int(r)] = proc[place], want_proc[place]
    check_marks(ctx, ad, seqs, inp, want, order=order)
    check_children(ctx, ad, seqs, inp, want, order=order)
    ad.close()


@pytest.mark.parametrize("nc", cases.CHILD_COUNTS)
def test_child_counts(ctx, nc):
    reads = cases.child_count_batch(nc)
    seqs = [cases.GEOMETRY_ADAPTER]
    want = wanted(seqs, 0, 1, 0, reads)
    assert sum(len(w[3]) for w in want) == nc
    ad = api.Adapters(seqs, errors=0, window=1, split_errors=0)
    check_marks(ctx, ad, seqs, reads, want)
    check_children(ctx, ad, seqs, reads, want, params=api.make_params(window_size=2))
    ad.close()


@pytest.mark.parametrize("n", cases.READ_COUNTS)
def test_read_counts(ctx, n):
    reads = cases.read_count_batch(n)
    seqs = [cases.GEOMETRY_ADAPTER]
    want = wanted(seqs, 0, 1, 0, reads)
    ad = api.Adapters(seqs, errors=0, window=1, split_errors=0)
    check_marks(ctx, ad, seqs, reads, want)
    got = check_children(ctx, ad, seqs, reads, want, params=api.make_params(window_size=5))
    assert len(got["child_ranges"]) >= 2 * (n // 3)
    ad.close()
