"""flx_adapter_cuts at the LAUNCH GEOMETRY the content tests of test_adapters_gpu.py never reach, against tests/_adapters_model.py for
equality.  The batches come from tests/_geometry_cases.py (tests/test_geometry_cases.py proves on a CPU that they are what is said
here).  A workgroup of k_adapter_cuts (csrc/adapters.hip) takes epb = min(kItemsPerGroup / P, kLdsTextBytes / round_up(W, 16),
kMaxEnds) read ends; what each case is the first test to execute:

  p2_w16      epb 512  the second round of the staging loop `le += kThreads` (s_n / s_read from kThreads on hold reads), full
  p2_w64      epb 512  the same where kItemsPerGroup / P and kLdsTextBytes / stride coincide: the dynamic LDS is all of kLdsTextBytes
  p2_w65      epb 409  a partial second staging round; an odd epb: `(e0 + le) & 1` starts a workgroup on a tail, one read's head and
                       tail are staged by different workgroups
  p4_w16      epb 256  exactly one staging round (le < epb ends with kThreads)
  p2_w150     epb 204  the default window with one sequence in more than one workgroup (blockIdx.x > 0 with P = 2)
  p6_w150     epb 170  the set of test_windows_and_errors in more than one workgroup
  p2_w1024    epb 32   the LDS-bound widest window in more than one workgroup: e0 > 0 with stride 1024
  p64_w1024   epb 16   items = epb * P = kItemsPerGroup at the widest window, several workgroups
  p256_w1024  epb 4    the smallest epb: two reads a workgroup

each as three batches: at least three workgroups with a partial last one (`ge < a.n_ends` fails inside a workgroup that has reads),
n_ends an exact multiple of epb (it never fails), and n_ends < epb (one partial workgroup; at epb 512 its second staging round holds
reads).  Both sides of every workgroup boundary hold a hit, every workgroup a hit and a miss.  Every batch runs with order = NULL and
with a random permutation under which the PROCESSING order, which is what the workgroups cut, stays the designed one.

Planes are filled with the adapter's own sequence between the reads, and every call goes through the host-array form, which prefills
the keys with 0xA5 (test_adapters_gpu.py)."""
import numpy as np
import pytest

import _adapters_cases as cases
import _adapters_model as model
import _geometry_cases as geo
from filtlong_amd import api

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


def run(ctx, ad, seqs, reads, order=None):
    plane, offsets, lengths = cases.pack(reads, fill=bytes(seqs[0]).upper())
    return ctx.adapter_cuts(plane, offsets, lengths, ad, order=order)


def same(got, want, reads):
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, [(int(i), len(reads[i]), got[i].tolist(), want[i].tolist()) for i in bad[:8]]


def check(ctx, name, kind):
    seqs, w, errors, epb, proc = geo.adapter_batch(name, kind)
    want = geo.adapter_keys(name, proc)  # model.keys_of, one end_key per distinct text
    ad = api.Adapters(seqs, errors=errors, window=w)
    try:
        assert len(ad) == len(model.patterns(seqs)) and geo.groups_of(len(ad), w) == epb
        same(run(ctx, ad, seqs, proc), want, proc)
        order = np.random.default_rng(len(proc)).permutation(len(proc)).astype(np.uint32)
        inp = geo.arrange(proc, order)  # the read processed at place i is still proc[i]
        want_inp = np.zeros_like(want)
        want_inp[order] = want
        same(run(ctx, ad, seqs, inp, order=order), want_inp, inp)
    finally:
        ad.close()
    return want


@pytest.mark.parametrize("kind", geo.ADAPTER_KINDS)
@pytest.mark.parametrize("name", [c[0] for c in geo.ADAPTER_CASES])
def test_workgroup_cuts(ctx, name, kind):
    want = check(ctx, name, kind)
    assert (want > 0).any() and (want == 0).any()


def test_one_context_shrinking_and_growing(ctx):
    """the largest batch, a one-read batch, a batch without a hit, the largest again: nothing of a larger call is left in a smaller"""
    name = "p2_w16"
    seqs, w, errors, epb, proc = geo.adapter_batch(name, "partial")
    assert len(proc) == max(geo.adapter_reads_of(c[3], k) for c in geo.ADAPTER_CASES for k in geo.ADAPTER_KINDS)
    want = geo.adapter_keys(name, proc)
    pool = geo.adapter_pool(name)
    quiet = [r for r in pool["none"]] * 3
    want_quiet = geo.adapter_keys(name, quiet)
    assert (want_quiet == 0).all() and (want > 0).sum() > 100
    ad = api.Adapters(seqs, errors=errors, window=w)
    try:
        same(run(ctx, ad, seqs, proc), want, proc)
        for one in (pool["both"][0], pool["none"][3], b""):
            same(run(ctx, ad, seqs, [one]), geo.adapter_keys(name, [one]), [one])
        same(run(ctx, ad, seqs, quiet), want_quiet, quiet)
        same(run(ctx, ad, seqs, proc), want, proc)
    finally:
        ad.close()
