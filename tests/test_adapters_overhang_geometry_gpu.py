"""flx_adapter_cuts of an object with O = 8 at the launch geometry of k_adapter_cuts, against tests/_adapters_overhang_model.py for
equality.  The batches are those of tests/_geometry_cases.py (whose CPU test proves what they are) with every whole adapter at a read
end replaced by a TRUNCATED one, so that both sides of every workgroup boundary hold a hit only the anchored walk finds:

  p2_w65      epb 409  an odd epb: a workgroup starts on a tail, one read's head and tail are staged by different workgroups
  p2_w1024    epb 32   the LDS-bound widest window in more than one workgroup (the anchored walk stops after m + k' of 1024 columns)
  p256_w1024  epb 4    the smallest epb, 256 patterns: every lane of a workgroup walks twice
  p6_w150     epb 170  three pattern lengths, 12 among them: lanes with and without a second walk in one wave

each as the three batches of the geometry tests, with order = NULL and with a random permutation under which the processing order
stays the designed one."""
import numpy as np
import pytest

import _adapters_cases as cases
import _adapters_overhang_model as model
import _geometry_cases as geo
from filtlong_amd import api

pytestmark = pytest.mark.gpu
OVERHANG = 8
NAMES = ("p2_w65", "p2_w1024", "p256_w1024", "p6_w150")
KEY_CACHE = {}  # case name -> {(side, text): key}


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


def truncated(name, proc, epb):
    """the designed reads with the first adapter's occurrences AT a read's edge cut by 6 to 8 bases (more than the free walk's
    allowance): the head loses the adapter's first bases, the tail (the reverse complement) its last.  The two read ends on either
    side of every workgroup boundary get such a remnant whatever they held"""
    a = bytes(geo.adapter_seqs(geo.adapter_case(name))[0]).upper()
    rc = model.revcomp(a)
    at_boundary = {e for b in range(epb, 2 * len(proc), epb) for e in (b - 1, b)}
    w = geo.adapter_case(name)[2]
    out = []
    for i, r in enumerate(proc):
        x = 6 + i % 3
        head, tail = 2 * i in at_boundary, 2 * i + 1 in at_boundary
        if head or tail:  # the window at that end goes, the remnant and W bases that match nothing come in
            r = r[w:] if head else r
            r = r[:max(len(r) - w, 0)] if tail else r
            r = (a[x:] + b"N" * w if head else b"") + r + (b"N" * w + rc[:len(rc) - x] if tail else b"")
        else:
            if r.startswith(a) and len(r) > len(a):
                r = r[x:]
            if r.endswith(rc) and len(r) > len(rc):
                r = r[:len(r) - x]
        out.append(r)
    return out


def same(got, want, reads):
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, [(int(i), len(reads[i]), got[i].tolist(), want[i].tolist()) for i in bad[:8]]


def run(ctx, ad, seqs, reads, order=None):
    plane, offsets, lengths = cases.pack(reads, fill=bytes(seqs[0]).upper())
    return ctx.adapter_cuts(plane, offsets, lengths, ad, order=order)


@pytest.mark.parametrize("kind", geo.ADAPTER_KINDS)
@pytest.mark.parametrize("name", NAMES)
def test_workgroup_cuts_with_overhang(ctx, name, kind):
    seqs, w, errors, epb, proc = geo.adapter_batch(name, kind)
    proc = truncated(name, proc, epb)
    pats = model.patterns(seqs)
    cache = KEY_CACHE.setdefault(name, {})
    want, plain = model.keys_of(proc, w, pats, errors, OVERHANG, cache, with_plain=True)
    assert (want >= plain).all() and (want > plain).any() and (want == 0).any()
    # both sides of every workgroup boundary: the end in front of it and the end behind it hold a hit that needs the overhang
    flat, flat_plain = want.reshape(-1), plain.reshape(-1)
    for b in range(epb, flat.size, epb):
        assert flat[b - 1] > flat_plain[b - 1] and flat[b] > flat_plain[b], (name, kind, b)
    ad = api.Adapters(seqs, errors=errors, window=w, overhang=OVERHANG)
    try:
        assert geo.groups_of(len(ad), w) == epb
        same(run(ctx, ad, seqs, proc), want, proc)
        order = np.random.default_rng(len(proc)).permutation(len(proc)).astype(np.uint32)
        inp = geo.arrange(proc, order)  # the read processed at place i is still proc[i]
        want_inp = np.zeros_like(want)
        want_inp[order] = want
        same(run(ctx, ad, seqs, inp, order=order), want_inp, inp)
    finally:
        ad.close()
