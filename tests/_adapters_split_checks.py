"""What the GPU tests of --split_adapters share: the model's answers for a batch, and the comparison of the library's marks and
children with them, for equality."""
import numpy as np

import _adapters_model as model
import _adapters_split_cases as cases
import _adapters_split_model as split
from filtlong_amd import api, synth


def quals_of(reads, seed=500):
    return [synth.qual_read(seed + i, len(r)).tobytes() if len(r) else b"" for i, r in enumerate(reads)]


def wanted(seqs, errors, window, e2, reads):
    pats = model.patterns(seqs)
    return [split.split_of(r, window, pats, errors, e2) for r in reads]


def pack_trapped(reads, seq):
    """cases.pack, with the bytes behind every read (its padding and any gap up to the next read) holding the adapter `seq` from its
    FIRST base on, repeated: a kernel that read on past a read's last base would walk into a whole occurrence at once"""
    seq = np.frombuffer(bytes(seq).upper(), dtype=np.uint8)
    plane, offsets, lengths = cases.pack(reads, fill=bytes(seq))
    ends = sorted(int(o) + int(n) for o, n in zip(offsets, lengths))
    starts = sorted(int(o) for o in offsets) + [plane.nbytes]
    for e in ends:
        nxt = min(s for s in starts if s >= e)
        if nxt > e:
            plane[e:nxt] = np.resize(seq, nxt - e)
    return plane, offsets, lengths


def check_marks(ctx, ad, seqs, reads, want, order=None):
    plane, offsets, lengths = pack_trapped(reads, seqs[0])
    got = ctx.adapter_marks(plane, offsets, lengths, ad, order=order)
    for i, (g, w) in enumerate(zip(got, want)):
        assert (g == w[2]).all(), (i, len(reads[i]), np.nonzero(g != w[2])[0][:8].tolist())
    words = ctx.adapter_marks(plane, offsets, lengths, ad, order=order, bitmap=True)
    assert len(words) == (plane.nbytes + 31) // 32
    assert int(np.unpackbits(words.view(np.uint8)).sum()) == sum(int(w[2].sum()) for w in want)  # nothing outside the reads


def check_children(ctx, ad, seqs, reads, want, order=None, params=None, child_capacity=None):
    splane, offsets, lengths = pack_trapped(reads, seqs[0])
    qplane, qoff, _ = cases.pack(quals_of(reads))
    assert (qoff == offsets).all()
    params = params or api.make_params(window_size=50, min_length=100)
    got = ctx.score_reads(qplane, offsets, lengths, params, order=order, adapters=ad, seq_plane=splane, child_capacity=child_capacity)
    children, coff = [], [0]
    for i, w in enumerate(want):
        assert (got["first"][i], got["last"][i]) == (w[4], w[5]), (i, len(reads[i]), got["first"][i], got["last"][i], w[4], w[5])
        children += w[3]
        coff.append(len(children))
    assert got["child_offsets"].tolist() == coff
    assert got["child_ranges"].tolist() == [list(c) for c in children]
    return got


def check(ctx, seqs, errors, window, e2, reads, order=None):
    want = wanted(seqs, errors, window, e2, reads)
    ad = api.Adapters(seqs, errors=errors, window=window, split_errors=e2)
    check_marks(ctx, ad, seqs, reads, want, order=order)
    check_children(ctx, ad, seqs, reads, want, order=order)
    ad.close()
    return want
