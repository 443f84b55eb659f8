"""flx_screenset and flx_screenset_hits against tests/_screen_k_model.py, for equality, at K = 17, 24 and 31 (and 16 against the
bitmap): the set after one and many batches, growth from 16 slots, duplicates and concurrent inserts of one key, either strand,
palindromes, sequence junctions and N; then the reads of test_screen_gpu.py with the edges moved to K — span and step edges, every
byte value, substitutions and indels, orders, 128-byte starts, no stale state.  The bytes between the reads of a plane are filled with
the contaminant's own sequence: a kernel that counted a window beyond a read's last base would find members there."""
import numpy as np
import pytest

import _screen_k_model as model
from filtlong_amd import api

pytestmark = pytest.mark.gpu
S = api.screen_span()
KS = (17, 24, 31)
STATE = 4  # FLX_ERR_STATE


def edge_lengths(k):
    return sorted(set(list(range(0, k + 18)) + [1023 + k - 2, 1023 + k - 1, 1023 + k, 1023 + k + 1, 2048 + k - 1, S + k - 3, S + k - 2, S + k - 1,
                                               2 * S + k - 1]))


def pack(reads, fill, align=16):
    """the plane of flx_score_batch with every byte that is not a read's taken from `fill`; starts on multiples of `align` for reads
    of at least 1024 bases when align > 16"""
    offsets, at = [], 0
    for r in reads:
        a = align if len(r) >= 1024 else 16
        at = (at + a - 1) // a * a
        offsets.append(at)
        at += (len(r) + 15) // 16 * 16
    plane = np.frombuffer((fill * (at // len(fill) + 1))[:at], dtype=np.uint8).copy() if at else np.zeros(0, dtype=np.uint8)
    for r, o in zip(reads, offsets):
        plane[o:o + len(r)] = np.frombuffer(r, dtype=np.uint8)
    return plane, np.array(offsets, dtype=np.uint64), np.array([len(r) for r in reads], dtype=np.int32)


def indel(rng, seq):
    s = bytearray(seq)
    a = int(rng.integers(40, len(s) - 40))
    n = int(rng.integers(1, 4))
    if rng.integers(0, 2):
        s[a:a] = model.random_seq(rng, n)
    else:
        del s[a:a + n]
    return bytes(s)


def from_ref(rng, ref, length, rate):
    """a read of any length from a short reference: fragments of it, either strand, one after the other"""
    out = b""
    while len(out) < length:
        out += model.draw(rng, ref, min(len(ref), length - len(out), 3000), rate)
    return out


@pytest.fixture(scope="module")
def ref5k():
    return model.random_seq(np.random.default_rng(101), 5000)


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


def make_set(ctx, k, batches, log2_capacity=None):
    ss = api.ScreenSet(ctx, k, log2_capacity)
    for seqs in batches:
        ss.add_fasta(seqs)
    ss.finalize()
    return ss


@pytest.fixture(scope="module")
def sets5k(ctx, ref5k):
    """per K: the set of the 5 kbp reference, grown from 16 slots, and the model's"""
    made = {k: (make_set(ctx, k, [[ref5k]], 4), model.build_set([ref5k], k)) for k in KS}
    yield made
    for ss, _ in made.values():
        ss.close()


@pytest.fixture(scope="module")
def battery(ref5k):
    """per K: the reads and the fill of their plane"""
    made = {}
    for k in KS:
        rng = np.random.default_rng(7 + k)
        reads = []
        for n in edge_lengths(k):
            reads.append(from_ref(rng, ref5k, n, 0.0))
            if n >= k:
                reads.append(from_ref(rng, ref5k, n, 0.05))
        for rate in (0.0, 0.05, 0.20):
            for strand in (0, 1):
                reads.append(model.draw(rng, ref5k, 1500, rate, strand))
        for _ in range(4):
            reads.append(indel(rng, model.draw(rng, ref5k, 700)))
        for n in (40, 999, 5000, S + 1000):
            reads.append(model.random_seq(rng, n))  # unrelated
        every = bytearray(from_ref(rng, ref5k, 256 * 70, 0.0))  # every byte value, 70 bases apart
        for v in range(256):
            every[70 * v + 35] = v
        reads.append(bytes(every))
        reads.append(bytes(rng.permutation(np.arange(256, dtype=np.uint8).repeat(4))))
        reads.append(model.draw(rng, ref5k, 2000).lower())
        mixed = bytearray(model.draw(rng, ref5k, 2000))
        for i in rng.integers(0, 2000, size=700):
            mixed[i] |= 0x20
        reads.append(bytes(mixed))
        reads.append(ref5k[:1000] + model.random_seq(rng, 1000))  # a chimera
        reads.append(from_ref(rng, ref5k, 300000, 0.02))  # many spans of one read
        made[k] = reads
    return made


@pytest.fixture(scope="module")
def wanted(sets5k, battery):
    """the model's hits of the battery, computed once"""
    return {k: model.hits_many(sets5k[k][1], battery[k], k) for k in KS}


def check(ctx, ss, want, reads, fill, align=16, order=None):
    plane, offsets, lengths = pack(reads, fill, align)
    got = ctx.screenset_hits(plane, offsets, lengths, ss, order=order)
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, [(int(i), len(reads[i]), int(got[i]), int(want[i])) for i in bad[:10]]
    return got


def check_model(ctx, ss, x, k, reads, fill, **kw):
    return check(ctx, ss, model.hits_many(x, reads, k), reads, fill, **kw)


# ---- the set ----
@pytest.mark.parametrize("k", KS)
def test_one_batch_and_growth_from_16_slots(sets5k, k):
    ss, x = sets5k[k]
    assert len(ss) == len(x) == 5000 - k + 1  # (a random 5 kbp sequence repeats no K-mer and holds no K-mer's reverse complement)
    assert ss.k == k and ss.capacity >= 2 * len(ss) and ss.capacity & (ss.capacity - 1) == 0


@pytest.mark.parametrize("k", KS)
def test_many_batches_grow_a_dozen_times(ctx, k):
    rng = np.random.default_rng(300 + k)
    seqs = [model.random_seq(rng, k - 1 + (1 << i)) for i in range(15)]  # 1, 2, 4, ... windows: every batch doubles the set
    seqs += [seqs[9],                                # a sequence fed twice, in different batches
             model.revcomp(seqs[11]),                # the other strand adds nothing
             model.random_seq(rng, k - 1), b"",      # no window
             model.random_seq(rng, 500)]
    x = model.build_set(seqs, k)
    ss = api.ScreenSet(ctx, k, 4)
    try:
        capacities = [ss.capacity]
        for a in range(len(seqs)):
            ss.add_fasta(seqs[a:a + 1])
            capacities.append(ss.capacity)
            assert ss.capacity >= 2 * len(ss)
            if a < 10 or a >= 14:
                assert len(ss) == len(model.build_set(seqs[:a + 1], k))
        ss.add_fasta([])
        ss.finalize()
        assert capacities[0] == 16 and len(set(capacities)) >= 13 and capacities == sorted(capacities)  # a dozen growths
        assert len(ss) == len(x) == (1 << 15) - 1 + 500 - k + 1 < sum(model.windows(len(s), k) for s in seqs)
        reads = [seqs[9], seqs[11], seqs[16], seqs[13][:300] + model.random_seq(rng, 300), model.random_seq(rng, 2000)]
        got = check_model(ctx, ss, x, k, reads, seqs[12])
        assert int(got[0]) == 512 and int(got[1]) == int(got[2]) == 2048 and int(got[4]) == 0
    finally:
        ss.close()


@pytest.mark.parametrize("k", KS)
def test_one_key_inserted_thousands_of_times_at_once(ctx, k):
    seqs = [b"ACGT" * 5000]
    x = model.build_set(seqs, k)
    # the four rotations of (ACGT)n: the reverse complement of a window is a window again, rotated, so two keys at odd K, two or four at even K
    assert len(x) <= 4
    ss = make_set(ctx, k, [seqs, seqs], 4)
    try:
        assert len(ss) == len(x)
        got = check_model(ctx, ss, x, k, [b"ACGT" * 100, b"CGTA" * 100, b"TGCA" * 100], b"ACGT" * 16)
        assert list(got) == [400 - k + 1, 400 - k + 1, 0]
    finally:
        ss.close()


@pytest.mark.parametrize("k", KS)
def test_palindromes_short_sequences_and_junctions(ctx, k):
    rng = np.random.default_rng(500 + k)
    half = model.random_seq(rng, 40)
    pal = half + model.revcomp(half)  # its own reverse complement: every key appears on both strands; at even K the centre window is one
    a, b = model.random_seq(rng, 200), model.random_seq(rng, 200)
    short = [model.random_seq(rng, n) for n in (0, 1, k - 1, k - 1)]
    seqs = [pal, a, b] + short
    x = model.build_set(seqs, k)
    assert len(x) == (80 - k + 2) // 2 + 2 * (200 - k + 1)
    ss = make_set(ctx, k, [seqs], 4)
    try:
        assert len(ss) == len(x)
        # the sequences were handed over back to back: a window across the junction of a and b is in X only if windows crossed it
        joined = a + b
        got = check_model(ctx, ss, x, k, [joined, pal, short[2] + short[3]], a)
        assert int(got[0]) == 2 * (200 - k + 1) and int(got[1]) == 80 - k + 1 and int(got[2]) == 0
    finally:
        ss.close()


@pytest.mark.parametrize("k", KS)
def test_n_every_k_bases_and_n_runs(ctx, ref5k, k):
    holes = bytearray(ref5k)
    holes[3::k] = b"N" * len(holes[3::k])
    ss = make_set(ctx, k, [[bytes(holes), bytes(holes).lower()]], 4)
    try:
        assert len(ss) == 0 == len(model.build_set([bytes(holes)], k))
        plane, offsets, lengths = pack([ref5k[:100]], ref5k)
        with pytest.raises(api.FlxError) as e:
            ctx.screenset_hits(plane, offsets, lengths, ss)
        assert e.value.code == STATE  # an empty set
    finally:
        ss.close()
    rng = np.random.default_rng(41)
    a, b = model.random_seq(rng, 600), model.random_seq(rng, 600)
    contaminant = [a + b"N" * 200 + b + b"NNN" + b"ACGTTGCAAGGCTAA" + b"n" * 50]
    x = model.build_set(contaminant, k)
    assert len(x) == 2 * (600 - k + 1)
    ss = make_set(ctx, k, [contaminant], 4)
    try:
        assert len(ss) == len(x)
        poly = [b"A" * 500, b"T" * 500, b"a" * 64, model.random_seq(rng, 300) + b"A" * 300, a[:300] + b"A" * 100, b"N" * 400]
        got = check_model(ctx, ss, x, k, poly, a)
        assert list(got[:4]) == [0, 0, 0, 0] and 300 - k + 1 <= int(got[4]) < 300 and int(got[5]) == 0
    finally:
        ss.close()


def test_state_errors(ctx, ref5k):
    plane, offsets, lengths = pack([ref5k[:100]], ref5k)
    ss = api.ScreenSet(ctx, 24, 4)
    try:
        ss.add_fasta([ref5k])
        with pytest.raises(api.FlxError) as e:  # not finalized
            ctx.screenset_hits(plane, offsets, lengths, ss)
        assert e.value.code == STATE
        ss.finalize()
        assert int(ctx.screenset_hits(plane, offsets, lengths, ss)[0]) == 100 - 23
        n, cap = len(ss), ss.capacity
        for call in (lambda: ss.add_fasta([ref5k]), lambda: ss.add_fasta([]), ss.finalize):
            with pytest.raises(api.FlxError) as e:
                call()
            assert e.value.code == STATE
        assert (len(ss), ss.capacity, ss.k) == (n, cap, 24)
    finally:
        ss.close()
    for k in (15, 32, 0, -1):
        with pytest.raises(api.FlxError) as e:
            api.ScreenSet(ctx, k)
        assert e.value.code == 1  # FLX_ERR_INVALID


# ---- the reads ----
@pytest.mark.parametrize("k", KS)
def test_battery(ctx, sets5k, ref5k, battery, wanted, k):
    ss, x = sets5k[k]
    reads, want = battery[k], wanted[k]
    got = check(ctx, ss, want, reads, ref5k)
    assert ctx.last_screen_filter() == "hash"
    by_len = {len(r): int(h) for r, h in zip(reads, got)}  # (of one length the later read wins: the mutated one)
    exact = {len(r): int(h) for r, h in zip(reads[::-1], got[::-1])}             # ... and here the first: the exact copy
    assert exact[k - 1] == 0 and exact[k] == 1 and exact[k + 17] == 18 and exact[0] == 0
    assert exact[S + k - 1] >= S - 200 and exact[2 * S + k - 1] >= 2 * S - 400 and by_len[S + k - 1] < S
    assert got[-1] > 50000
    again = check(ctx, ss, want, reads, ref5k)  # a second call on the same context: the same hits, nothing accumulated
    assert (again == got).all()


@pytest.mark.parametrize("k", KS)
def test_order_and_128_byte_starts(ctx, sets5k, ref5k, battery, wanted, k):
    ss, _ = sets5k[k]
    reads, want = battery[k], wanted[k]
    _, _, lengths = pack(reads, ref5k)
    check(ctx, ss, want, reads, ref5k, order=api.length_order(lengths))
    check(ctx, ss, want, reads, ref5k, order=api.length_order(lengths)[::-1].copy())
    check(ctx, ss, want, reads, ref5k, order=np.random.default_rng(5).permutation(len(reads)).astype(np.uint32))
    check(ctx, ss, want, reads, ref5k, align=128)
    check(ctx, ss, want, reads, ref5k, align=128, order=api.length_order(lengths)[::-1].copy())


@pytest.mark.parametrize("k", KS)
def test_substitutions_strands_and_unrelated(ctx, sets5k, ref5k, k):
    ss, x = sets5k[k]
    rng = np.random.default_rng(23 + k)
    reads, kinds = [], []
    for rate in (0.0, 0.05, 0.20):
        for strand in (0, 1):
            for _ in range(6):
                reads.append(model.draw(rng, ref5k, int(rng.integers(200, 4000)), rate, strand))
                kinds.append((rate, strand))
    for _ in range(12):
        reads.append(indel(rng, model.draw(rng, ref5k, int(rng.integers(400, 3000)))))
        kinds.append(("indel", 0))
    for _ in range(12):
        reads.append(model.random_seq(rng, int(rng.integers(k, 6000))))
        kinds.append(("unrelated", 0))
    got = check_model(ctx, ss, x, k, reads, ref5k)
    frac = {kind: [] for kind in set(kinds)}
    for r, kind, h in zip(reads, kinds, got):
        frac[kind].append(int(h) / (len(r) - k + 1))
    for strand in (0, 1):
        assert min(frac[(0.0, strand)]) == 1.0                                             # every window of an exact copy, on either strand
        assert 0.6 * 0.95 ** k < np.mean(frac[(0.05, strand)]) < 1.5 * 0.95 ** k            # (1 - e)^K of the windows survive
        assert np.mean(frac[(0.20, strand)]) < 3 * 0.8 ** k + 0.002
    assert min(frac[("indel", 0)]) > 0.85 and max(frac[("indel", 0)]) < 1.0                 # the windows across the indel are lost
    assert max(frac[("unrelated", 0)]) == 0.0                                              # |X| / 4^K is below 1e-6


@pytest.mark.parametrize("k", KS)
def test_every_byte_value_and_lowercase(ctx, sets5k, ref5k, k):
    ss, x = sets5k[k]
    reads = []
    for v in range(256):  # one read per byte value: a copy of X with that byte at three places
        s = bytearray(ref5k[100:300])
        for at in (0, 77, 199):
            s[at] = v
        reads.append(bytes(s))
    reads.append(ref5k.lower())
    reads.append(ref5k)
    got = check_model(ctx, ss, x, k, reads, ref5k)
    assert int(got[-1]) == int(got[-2]) == 5000 - k + 1
    assert int(got[ord("N")]) == 200 - k + 1 - (1 + k + 1) and int(got[ord("n")]) == int(got[ord("N")])
    for c in b"ACGTacgt":
        assert int(got[c]) >= 200 - k + 1 - (1 + k + 1)


def test_k16_is_the_bitmap(ctx, ref5k):
    """at K = 16 the hashed set answers what the exact bitmap of flx_screen_hits answers, on the same reads"""
    rng = np.random.default_rng(16)
    contaminant = [ref5k, model.random_seq(rng, 700) + b"NN" + model.random_seq(rng, 300), b"ACGTACGTACGTACG"]
    reads = [from_ref(rng, ref5k, n, rate) for n in edge_lengths(16)[::3] for rate in (0.0, 0.05)]
    reads += [model.random_seq(rng, 3000), contaminant[1], model.revcomp(contaminant[1]), from_ref(rng, ref5k, 3 * S + 100, 0.03)]
    ks = api.Kmers(ctx)
    ks.add_screen_fasta(contaminant)
    ks.finalize()
    ss = make_set(ctx, 16, [contaminant], 4)
    try:
        plane, offsets, lengths = pack(reads, ref5k)
        want = ctx.screen_hits(plane, offsets, lengths, ks)
        got = ctx.screenset_hits(plane, offsets, lengths, ss)
        assert (got == want).all() and int(want.sum()) > 10000
        assert ctx.last_screen_filter() == "hash"
        x = model.build_set(contaminant, 16)
        assert len(ss) == len(x) and (got == model.hits_many(x, reads, 16)).all()
    finally:
        ks.close()
        ss.close()
