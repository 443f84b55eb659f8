"""flx_screen_hits against tests/_screen_model.py, for equality: the span and step edges of k_screen_hits, every byte value, either
strand, substitutions and indels, the ACGT splitter's reason (N runs against poly-A), the three filter forms on the same reads, and no
stale state between calls.  The bytes between the reads of a plane (the padding up to 16, and any gap behind it) are filled with the
contaminant's own sequence: a kernel that counted a window beyond a read's last base would find members there."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import _screen_model as model
from filtlong_amd import api

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = api.screen_span()
EDGE_LENGTHS = [0, 1, 15, 16, 17, 31, 32, 33, 1023, 1024, 1025, 1038, 1039, 1040, 1041, 2048 + 15, S + 14, S + 15, S + 16, 2 * S + 15]


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
    a = int(rng.integers(20, len(s) - 20))
    k = int(rng.integers(1, 4))
    if rng.integers(0, 2):
        s[a:a] = model.random_seq(rng, k)
    else:
        del s[a:a + k]
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
def battery(ref5k):
    """the reads every filter form is asked about"""
    rng = np.random.default_rng(7)
    reads = []
    for n in EDGE_LENGTHS:
        reads.append(from_ref(rng, ref5k, n, 0.0))
        reads.append(from_ref(rng, ref5k, n, 0.05))
    for rate in (0.0, 0.05, 0.20):
        for strand in (0, 1):
            reads.append(model.draw(rng, ref5k, 1500, rate, strand))
    for _ in range(4):
        reads.append(indel(rng, model.draw(rng, ref5k, 700)))
    for n in (40, 999, 5000, S + 1000):
        reads.append(model.random_seq(rng, n))  # unrelated
    every = bytearray(from_ref(rng, ref5k, 256 * 40, 0.0))  # every byte value, 40 bases apart
    for v in range(256):
        every[40 * v + 20] = v
    reads.append(bytes(every))
    reads.append(bytes(rng.permutation(np.arange(256, dtype=np.uint8).repeat(4))))
    reads.append(model.draw(rng, ref5k, 2000).lower())
    mixed = bytearray(model.draw(rng, ref5k, 2000))
    for i in rng.integers(0, 2000, size=700):
        mixed[i] |= 0x20
    reads.append(bytes(mixed))
    reads.append(ref5k[:1000] + model.random_seq(rng, 1000))  # a chimera
    reads.append(from_ref(rng, ref5k, 300000, 0.05))  # many spans of one read
    return reads


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


def make_set(ctx, seqs):
    ks = api.Kmers(ctx)
    ks.add_screen_fasta(seqs)
    ks.finalize()
    return ks


@pytest.fixture(scope="module")
def set5k(ctx, ref5k):
    ks = make_set(ctx, [ref5k])
    yield ks, model.build_set([ref5k])
    ks.close()


def check(ctx, ks, x, reads, fill, align=16, order=None):
    plane, offsets, lengths = pack(reads, fill, align)
    got = ctx.screen_hits(plane, offsets, lengths, ks, order=order)
    want = np.array([model.hits(x, r) for r in reads], dtype=np.uint32)
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, [(int(i), len(reads[i]), int(got[i]), int(want[i])) for i in bad[:10]]
    return got


def test_set_is_the_model_set(ctx, set5k, ref5k):
    ks, x = set5k
    assert len(ks) == len(x)
    rng = np.random.default_rng(2)
    q = np.unique(np.concatenate([x[::7], rng.integers(0, 1 << 32, size=5000, dtype=np.uint64).astype(np.uint32)]))
    assert (ks.is_kmer_present(q) == np.isin(q, x)).all()


def test_battery_lds_form(ctx, set5k, ref5k, battery):
    ks, x = set5k
    got = check(ctx, ks, x, battery, ref5k)
    assert ctx.last_screen_filter() == "lds"
    # the battery is what it claims: whole-read matches on the edges, nothing in a read below 16 bases, hits on both strands
    by_len = {len(r): int(h) for r, h in zip(battery[:2 * len(EDGE_LENGTHS):2], got[:2 * len(EDGE_LENGTHS):2])}
    assert by_len[S + 15] >= S - 200 and by_len[2 * S + 15] >= 2 * S - 400 and by_len[15] == 0 and by_len[16] == 1
    assert got[-1] > 50000 and int(got[-1]) == model.hits(x, battery[-1])
    # a second call on the same context: the same hits, nothing accumulated
    again = check(ctx, ks, x, battery, ref5k)
    assert (again == got).all()


def test_order_and_128_byte_starts(ctx, set5k, ref5k, battery):
    ks, x = set5k
    _, _, lengths = pack(battery, ref5k)
    check(ctx, ks, x, battery, ref5k, order=api.length_order(lengths))
    check(ctx, ks, x, battery, ref5k, order=np.random.default_rng(5).permutation(len(battery)).astype(np.uint32))
    check(ctx, ks, x, battery, ref5k, align=128)
    check(ctx, ks, x, battery, ref5k, align=128, order=api.length_order(lengths)[::-1].copy())


def test_substitutions_strands_and_unrelated(ctx, set5k, ref5k):
    ks, x = set5k
    rng = np.random.default_rng(23)
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
        reads.append(model.random_seq(rng, int(rng.integers(16, 6000))))
        kinds.append(("unrelated", 0))
    got = check(ctx, ks, x, reads, ref5k)
    frac = {k: [] for k in set(kinds)}
    for r, k, h in zip(reads, kinds, got):
        frac[k].append(int(h) / (len(r) - 15))
    for strand in (0, 1):
        assert min(frac[(0.0, strand)]) == 1.0                                  # every window of an exact copy, on either strand
        assert 0.3 < np.mean(frac[(0.05, strand)]) < 0.6                        # 0.95^16 = 0.44
        assert 0.005 < np.mean(frac[(0.20, strand)]) < 0.08                     # 0.8^16 = 0.028
    assert min(frac[("indel", 0)]) > 0.9 and max(frac[("indel", 0)]) < 1.0      # the windows across the indel are lost
    assert max(frac[("unrelated", 0)]) < 0.01                                   # |X| / 2^32 = 2e-6


def test_every_byte_value_and_lowercase(ctx, set5k, ref5k):
    ks, x = set5k
    rng = np.random.default_rng(31)
    reads = []
    for v in range(256):  # one read per byte value: a copy of X with that byte at three places
        s = bytearray(ref5k[100:300])
        for at in (0, 77, 199):
            s[at] = v
        reads.append(bytes(s))
    reads.append(ref5k.lower())
    reads.append(ref5k)
    got = check(ctx, ks, x, reads, ref5k)
    assert int(got[-1]) == int(got[-2]) == 5000 - 15
    assert int(got[ord("N")]) == 200 - 15 - (1 + 16 + 1) and int(got[ord("n")]) == int(got[ord("N")])
    for c in b"ACGTacgt":
        assert int(got[c]) >= 200 - 15 - (1 + 16 + 1)
    # X's own sequence with one N every 16 bases has no window left
    holes = bytearray(ref5k)
    holes[3::16] = b"N" * len(holes[3::16])
    assert list(check(ctx, ks, x, [bytes(holes), bytes(holes).lower()], ref5k)) == [0, 0]


def test_n_runs_put_no_poly_a_into_the_set(ctx):
    """the reason for the splitter: flx_kmerset_add_assembly reads N as A, so an N run would make every poly-A tail a hit"""
    rng = np.random.default_rng(41)
    a, b = model.random_seq(rng, 600), model.random_seq(rng, 600)
    contaminant = [a + b"N" * 200 + b + b"NNN" + b"ACGTTGCAAGGCTAA" + b"n" * 50]  # (the last piece has 15 bases: dropped)
    x = model.build_set(contaminant)
    assert len(x) == 2 * 2 * (600 - 15)
    ks = make_set(ctx, contaminant)
    try:
        assert len(ks) == len(x)
        poly = [b"A" * 500, b"T" * 500, b"a" * 64, model.random_seq(rng, 300) + b"A" * 300, a[:300] + b"A" * 100, b"N" * 400]
        got = check(ctx, ks, x, poly, a)
        assert list(got[:4]) == [0, 0, 0, 0] and 300 - 15 <= int(got[4]) < 300 and int(got[5]) == 0
        # the same sequences handed over as they are DO hold poly-A: the splitter is what keeps it out
        raw = api.Kmers(ctx)
        raw.add_assembly_fasta(contaminant)
        raw.finalize()
        assert raw.is_kmer_present(np.array([0], dtype=np.uint32)).all()  # (N is code 0 on both strands' encoders)
        assert not ks.is_kmer_present(np.array([0, 0xFFFFFFFF], dtype=np.uint32)).any()
        raw.close()
    finally:
        ks.close()


def test_empty_and_unfinished_sets_are_a_state_error(ctx, ref5k):
    plane, offsets, lengths = pack([ref5k[:100]], ref5k)
    ks = make_set(ctx, [b"ACGTACGTACGTACG", b"ACGTACGNACGTACGTACGTAC", b""])  # no run of 16
    try:
        assert len(ks) == 0
        with pytest.raises(api.FlxError) as e:
            ctx.screen_hits(plane, offsets, lengths, ks)
        assert e.value.code == 4  # FLX_ERR_STATE
    finally:
        ks.close()
    ks = api.Kmers(ctx)
    try:
        ks.add_screen_fasta([ref5k])
        with pytest.raises(api.FlxError) as e:
            ctx.screen_hits(plane, offsets, lengths, ks)
        assert e.value.code == 4
    finally:
        ks.close()


def test_pre12_form_on_the_same_reads(ctx, ref5k, battery):
    """X of 2 Mbp (the 5 kbp contaminant inside it): its 10-mer table is full, the 12-mer prefilter stands alone in front of the bitmap"""
    big = [ref5k + model.random_seq(np.random.default_rng(55), 2000000 - 5000)]
    x = model.build_set(big)
    ks = make_set(ctx, big)
    try:
        assert len(ks) == len(x)
        got = check(ctx, ks, x, battery, ref5k)
        assert ctx.last_screen_filter() == "pre12"
        x5 = model.build_set([ref5k])
        assert all(int(g) >= model.hits(x5, r) for g, r in zip(got[:20], battery[:20]))
    finally:
        ks.close()


def test_exact_form_on_the_same_reads(ref5k, battery, tmp_path):
    """FLX_KMER_PREFILTER=0 is read when a set is finalized: a child process builds the set without prefilters and asks the bitmap alone"""
    src, dst = str(tmp_path / "in.npz"), str(tmp_path / "out.json")
    plane, offsets, lengths = pack(battery, ref5k)
    np.savez(src, ref=np.frombuffer(ref5k, dtype=np.uint8), plane=plane, offsets=offsets, lengths=lengths)
    env = dict(os.environ, FLX_KMER_PREFILTER="0", PYTHONPATH=ROOT)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_screen_worker.py"), src, dst], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=300)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    out = json.load(open(dst))
    assert out["filter"] == "exact"
    x = model.build_set([ref5k])
    assert out["hits"] == [model.hits(x, r) for r in battery]
