"""flx_endtrim_cuts at the edges of its LAUNCH GEOMETRY, against tests/_endtrim_model.py for equality.

k_endtrim_spans (csrc/endtrim.hip) is persistent: 5 workgroups of 4 waves per CU walk the spans with `sp += n_waves`; a span is
endtrim_span() quality bytes of one read, taken 1024 a step, every lane one aligned 16-byte load; k_endtrim_reads combines the spans of
a read, one wave per read.

  the phases   a read's offset is a multiple of 16 by the plane's rule (flx_plane_layout; the library refuses any other), so "every
               offset" is every 16-byte phase of a 256-byte row: the same read sixteen times in one plane, each copy one phase
               further, with lengths of every residue mod 16 (where the last load of a read ends) — one read of a few steps and one
               of more than a span
  the end      the same read as the LAST read of a plane that ends with the read's last 16-byte slot: the loads stay inside it
  the chunks   the batch in chunks of 1, 3 and all reads gives equal cuts (a read's cuts do not depend on its neighbours)
  the crowd    more than twice the short reads of one pass of the grid's waves (sized from device_info()["n_cu"]), so every wave comes
               round `sp += n_waves` a second time; reads without a base (no span: equal neighbours in the segment table) among them,
               and reads of several spans at the start and the end

each with order NULL and, where it says so, the length order and a random permutation."""
import numpy as np
import pytest

import _endtrim_cases as cases
import _endtrim_model as model
from filtlong_amd import api

pytestmark = pytest.mark.gpu
WAVES_PER_CU = 5 * 4  # csrc/endtrim.hip: kEndtrimBlocksPerCU workgroups of kEndtrimThreads / 64 waves


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


def place(reads, phases=None, tail=0):
    """a plane by hand: read i at the next offset whose 16-byte phase in a 256-byte row is phases[i] (None: the next slot); `tail`
    bytes behind the last read's last slot"""
    offsets, at = [], 0
    for i, r in enumerate(reads):
        if phases is not None:
            while (at // 16) % 16 != phases[i]:
                at += 16
        offsets.append(at)
        at += (len(r) + 15) // 16 * 16
    plane = np.zeros(max(at + tail, 16), dtype=np.uint8)
    for r, o in zip(reads, offsets):
        plane[o:o + len(r)] = np.frombuffer(r, dtype=np.uint8)
    return plane, np.array(offsets, dtype=np.uint64), np.array([len(r) for r in reads], dtype=np.int32)


def test_every_phase_and_every_residue(ctx):
    span = api.endtrim_span()
    rng = np.random.default_rng(21)
    for base in (cases.ont_like(rng, 3 * 1024 + 16, 300, 700), cases.ont_like(rng, span + 2048 + 16, 1500, 40)):
        reads = [base[8:len(base) - k] for k in range(16)]  # sixteen lengths, one of every residue mod 16
        want = model.batch_cuts(reads, cases.T90)
        assert sorted(len(r) % 16 for r in reads) == list(range(16)) and (want > 0).all()
        plane, offsets, lengths = place(reads, phases=list(range(16)))
        assert sorted(int(o) // 16 % 16 for o in offsets) == list(range(16))
        got = ctx.endtrim_cuts(plane, offsets, lengths, cases.T90)
        assert (got == want).all(), np.flatnonzero((got != want).any(axis=1))
        same = [base] * 16  # ... and the SAME read at every phase: the same cuts sixteen times
        plane, offsets, lengths = place(same, phases=list(range(16)))
        got = ctx.endtrim_cuts(plane, offsets, lengths, cases.T90)
        assert (got == np.array(model.cuts(base, cases.T90), dtype=np.uint32)).all()


def test_the_last_read_of_a_plane(ctx):
    span = api.endtrim_span()
    rng = np.random.default_rng(22)
    for n in (1, 15, 16, 17, 1023, 1024, 1025, span - 1, span, span + 1, 2 * span + 1009):
        last = cases.ont_like(rng, n, min(n, 30), min(n, 20))
        reads = [cases.ont_like(rng, 500), b"", last]
        plane, offsets, lengths = place(reads, tail=0)
        assert int(offsets[-1]) + (n + 15) // 16 * 16 == plane.nbytes  # the plane ends with the read's last slot
        got = ctx.endtrim_cuts(plane, offsets, lengths, cases.T90)
        assert (got == model.batch_cuts(reads, cases.T90)).all(), n


def test_chunks_of_one_three_and_all(ctx):
    span = api.endtrim_span()
    rng = np.random.default_rng(23)
    reads = cases.mixed_batch(rng, 45, 4000) + [cases.ont_like(rng, span + 77, 200, 3000), b"", cases.ont_like(rng, 3 * span + 1, 0, 600)]
    want = model.batch_cuts(reads, cases.T90)
    for size in (1, 3, len(reads)):
        parts = []
        for a in range(0, len(reads), size):
            plane, offsets, lengths = api.pack_reads(reads[a:a + size])
            parts.append(ctx.endtrim_cuts(plane, offsets, lengths, cases.T90))
        got = np.concatenate(parts)
        assert (got == want).all(), (size, np.flatnonzero((got != want).any(axis=1))[:10])


def test_crowd_takes_a_second_trip(ctx):
    span = api.endtrim_span()
    n_waves = ctx.device_info()["n_cu"] * WAVES_PER_CU
    rng = np.random.default_rng(24)
    n = n_waves * 9 // 4
    lengths = rng.integers(1, 120, size=n)
    lengths[rng.integers(0, n, size=n // 50)] = 0  # no span
    lengths[:3] = (5, 0, 63)
    lengths[-3:] = (63, 0, 7)
    noise = cases.ont_like(rng, 8192, 0, 0)
    junk = cases.rand_bytes(rng, 200, 33, 40)
    reads = [cases.ont_like(rng, 2 * span + 500, 900, 100)]
    for i, L in enumerate(lengths):
        L = int(L)
        a = int(rng.integers(0, 8192 - 120))
        reads.append(junk[:L // 3] + noise[a:a + L - L // 3] if i % 2 else noise[a:a + L - L // 4] + junk[:L // 4])
    reads.append(cases.ont_like(rng, span + 99, 10, 2000))
    spans = sum((len(r) + span - 1) // span for r in reads)
    assert spans > 2 * n_waves + n_waves // 8  # every wave takes two spans, and more than an eighth of them a third
    want = model.batch_cuts(reads, cases.T90)
    plane, offsets, lens = api.pack_reads(reads)
    for order in (None, api.length_order(lens), rng.permutation(len(reads)).astype(np.uint32)):
        got = ctx.endtrim_cuts(plane, offsets, lens, cases.T90, order=order)
        bad = np.flatnonzero((got != want).any(axis=1))
        assert len(bad) == 0, (order is None, len(bad), [(int(i), len(reads[i]), got[i].tolist(), want[i].tolist()) for i in bad[:10]])
    assert (want[:, 0] > 0).sum() > len(reads) // 4 and (want[:, 1] > 0).sum() > len(reads) // 4
