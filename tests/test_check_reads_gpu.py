"""The host-array entry points refuse the same bad reads with the same words: flx_screen_hits, flx_screenset_hits, flx_adapter_cuts and
flx_score_batch share one check of the read layout (and, the first three, of `order`).  A refused call leaves the context usable: the
next good call answers the models' values."""
import numpy as np
import pytest

import _adapters_model as adapters_model
import _screen_k_model as model_k
import _screen_model as model
from filtlong_amd import api

pytestmark = pytest.mark.gpu
INVALID = 1  # FLX_ERR_INVALID

LAYOUT = "offset must be 16-byte aligned and inside the plane"
BAD = {  # name -> (what to break, the library's words)
    "negative length": (lambda o, l, order: (o, np.array([40, -1, 40], dtype=np.int32), order), "read 1: " + LAYOUT),
    "offset off the 16-byte grid": (lambda o, l, order: (o + np.array([0, 8, 0], dtype=np.uint64), l, order), "read 1: " + LAYOUT),
    "read beyond the plane": (lambda o, l, order: (o, np.array([40, 40, 64], dtype=np.int32), order), "read 2: " + LAYOUT),
    "order with a duplicate": (lambda o, l, order: (o, l, np.array([0, 0, 1], dtype=np.uint32)), "order is not a permutation of the reads"),
    "order with an entry >= n": (lambda o, l, order: (o, l, np.array([0, 1, 3], dtype=np.uint32)), "order is not a permutation of the reads"),
}


def test_one_check_of_the_reads_for_four_entry_points():
    rng = np.random.default_rng(77)
    ref = model.random_seq(rng, 5000)
    reads = [ref[100:140], model.revcomp(ref[2000:2040]), model.random_seq(rng, 40)]
    adapter = [model.random_seq(rng, 20)]
    reads[2] = adapter[0] + reads[2][20:]
    plane, offsets, lengths = api.pack_reads(reads)
    assert list(offsets) == [0, 48, 96] and plane.nbytes == 144
    ctx = api.Context(0)
    try:
        ks = api.Kmers(ctx)
        ks.add_screen_fasta([ref])
        ks.finalize()
        ss = api.ScreenSet(ctx, 24)
        ss.add_fasta([ref])
        ss.finalize()
        ad = api.Adapters(adapter, errors=20, window=150)
        params = api.make_params()
        calls = {
            "flx_screen_hits": lambda o, l, order: ctx.screen_hits(plane, o, l, ks, order=order),
            "flx_screenset_hits": lambda o, l, order: ctx.screenset_hits(plane, o, l, ss, order=order),
            "flx_adapter_cuts": lambda o, l, order: ctx.adapter_cuts(plane, o, l, ad, order=order),
            "flx_score_batch": lambda o, l, order: ctx.score_reads(plane, o, l, params, order=order),  # (the bases as quality bytes)
        }
        for name, (make, words) in BAD.items():
            said = {}
            for fn, call in calls.items():
                if fn == "flx_score_batch" and name.startswith("order"):
                    continue  # flx_score_batch takes any order
                with pytest.raises(api.FlxError) as e:
                    call(*make(offsets, lengths, None))
                assert e.value.code == INVALID, (name, fn)
                said[fn] = str(e.value)
            assert len(set(said.values())) == 1 and said["flx_screen_hits"].endswith(": " + words), (name, said)
        # the context after ten and more refusals
        want16 = model.hits_many(model.build_set([ref]), reads)
        want24 = model_k.hits_many(model_k.build_set([ref], 24), reads, 24)
        assert list(want16[:2]) == [25, 25] and list(want24[:2]) == [17, 17]
        order = np.array([2, 0, 1], dtype=np.uint32)
        assert (calls["flx_screen_hits"](offsets, lengths, order) == want16).all()
        assert (calls["flx_screenset_hits"](offsets, lengths, order) == want24).all()
        keys = adapters_model.keys_of(reads, 150, adapters_model.patterns(adapter), 20)
        assert (calls["flx_adapter_cuts"](offsets, lengths, order) == keys).all() and keys[2, 0] >> 8 == 20
        assert calls["flx_score_batch"](offsets, lengths, order)["passed"].all()
    finally:
        ctx.close()
