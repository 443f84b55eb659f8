"""k-mer mode: the window fold of ultra-long reads and children, one wave per segment (score_kmer_long.hip) — bit-identical to the
oracle and the reference binary.

Reads and children from a length threshold on (2^18 bases, raised with the batch's bases per lane; FLX_KMER_LONG_MIN=N forces N, 0
turns the path off) are left alone by the one-lane kernels (k_kmer_fold MODE 0 / 3 / 5 / 6) and folded cooperatively, where those
kernels would fold on the integer grid.  Whether the path ran is visible in flx_timing_get under "flx_score_kmer_long"."""
import os
import subprocess
import time

import numpy as np
import pytest

import _cases
import _oracle
from filtlong_amd import api, synth as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "filtlong_amd", "bin", "filtlong")
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
PERIODS = [(16, 16), (17, 15), (40, 40), (100, 20), (20, 100), (125, 125), (126, 124), (250, 250), (500, 300), (62, 190), (31, 219),
           (15, 235), (8, 242), (3000, 900), (1000, 16), (249, 1), (1, 16), (64, 64), (33, 31), (700, 700)]
SWITCHES = ("FLX_KMER_LONG_MIN", "FLX_KMER_FOLD", "FLX_KMER_FOLD_GRID", "FLX_KMER_FOLD_EVENTS")


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def kmers(ctx):
    """The reference set of tests/test_gpu_kmer.py::test_integer_grid_folds_vs_oracle: (reference bases, oracle set, device set)."""
    ref = S.bases_read(S.STREAM_REF, 0, 0, 400_000)
    oset = _oracle.KmerSet()
    oset.add_assembly([ref.tobytes()])
    ks = api.Kmers(ctx)
    ks.add_assembly_fasta([ref.tobytes()])
    ks.finalize()
    yield ref, oset, ks
    ks.close()


def junk(rng, n):
    return ACGT[rng.integers(0, 4, n)]


def low(n):
    """n bases with three distinct 16-mers, none of them in the set (random junk of some kbp holds a 16-mer of the set now and then)."""
    return np.frombuffer((b"ACG" * (n // 3 + 1))[:n], dtype=np.uint8).copy()


def cut_offs(want, lengths, pkw):
    """The oracle's scores under hard cut-offs: the pass flags of src/read.cpp:64-73 from the values it computed without them."""
    def ok(L, mean, window):
        return ((L >= pkw.get("min_length", 0)) & (L <= pkw.get("max_length", 1 << 31)) & (mean >= pkw.get("min_mean_q", -1.0))
                & (window >= pkw.get("min_window_q", -1.0))).astype(np.uint8)
    cr = want["child_ranges"]
    return dict(want, passed=ok(np.asarray(lengths), want["mean_q"], want["window_q"]),
                child_passed=ok(cr[:, 1] - cr[:, 0], want["child_mean_q"], want["child_window_q"]))


def tiled(ref, rng, L):
    """L bases tiled from the reference (pieces of 20-150 kbp from random places)."""
    out = []
    while sum(len(x) for x in out) < L:
        n = int(rng.integers(20_000, 150_000))
        s = int(rng.integers(0, len(ref) - n))
        out.append(ref[s:s + n])
    return np.concatenate(out)[:L].copy()


def score(ctx, ks, packed, pkw, order=None, env=None):
    """One scoring call under the given switches: (scores, launches of the cooperative path, launches of MODE 5)."""
    plane, offsets, lengths = packed
    with pytest.MonkeyPatch.context() as mp:
        for k in SWITCHES:
            mp.delenv(k, raising=False)
        for k, v in (env or {}).items():
            mp.setenv(k, v)
        ctx.timing_enable(True)
        ctx.timing_reset()
        try:
            got = ctx.score_reads(plane, offsets, lengths, api.make_params(**pkw), kmers=ks, order=order, child_capacity=max(64, len(lengths)) * 40)
            return got, ctx.timing_get("flx_score_kmer_long")[1], ctx.timing_get("flx_score_kmer_fold.m5")[1]
        finally:
            ctx.timing_enable(False)


def oracle(oset, packed, pkw):
    plane, offsets, lengths = packed
    return _oracle.score_plane_mt(plane, offsets, lengths, _oracle.make_params(**pkw), kmerset=oset, child_cap=max(64, len(lengths)) * 40)


def orders(lengths, seed=3):
    return {None: None, "random": np.random.default_rng(seed).permutation(len(lengths)).astype(np.uint32), "desc": api.length_order(lengths)}


# ------------------------------------------------------------------------------------------------------------ 1. real length
@pytest.fixture(scope="module")
def real_batch(kmers):
    """Reads of 0.3 / 1 / 2.5 / 4 Mbp tiled from the reference with 3 % substitutions — junk blocks of 20-5000 bases (more than 8
    children), leading and trailing junk (trim), and in the 4 Mbp read one stretch of 300 kbp without junk or substitutions (a child
    that is long itself) — among 200 reads of up to 20 kbp."""
    ref = kmers[0]
    rng = np.random.default_rng(2024)
    reads = []
    for L in (300_000, 1_000_000, 2_500_000, 4_000_000):
        seq = tiled(ref, rng, L)
        sub = rng.random(L) < 0.03
        seq[sub] = junk(rng, int(sub.sum()))
        for _ in range(30 + L // 100_000):
            n = int(rng.choice([20, 40, 70, 300, 600, 2000, 5000]))
            p = int(rng.integers(0, L - n))
            seq[p:p + n] = junk(rng, n)
        if L == 4_000_000:
            s = int(rng.integers(0, len(ref) - 300_000))
            seq[1_700_000:2_000_000] = ref[s:s + 300_000]
        head, tail = int(rng.integers(30, 900)), int(rng.integers(30, 900))
        seq[:head] = junk(rng, head)
        seq[L - tail:] = junk(rng, tail)
        reads.append(seq.tobytes())
    for L in rng.integers(1, 20_000, 200):
        s = int(rng.integers(0, len(ref) - int(L)))
        seq = ref[s:s + int(L)].copy()
        sub = rng.random(int(L)) < 0.05
        seq[sub] = junk(rng, int(sub.sum()))
        if L > 3000:
            p = int(rng.integers(0, int(L) - 700))
            seq[p:p + 700] = junk(rng, 700)
        reads.append(seq.tobytes())
    return api.pack_reads(reads)


@pytest.mark.parametrize("extra", [dict(), dict(trim=True, split=500), dict(split=64)], ids=["plain", "trim+split500", "split64"])
@pytest.mark.parametrize("ws", [250, 500, 128])
def test_parity_at_real_length(ctx, kmers, real_batch, ws, extra):
    """At the default threshold: every field bit-identical to the oracle, without children, with --trim --split 500 and with
    --split 64, then with the hard cut-offs set to the oracle's exact values; the cooperative path ran."""
    _ref, oset, ks = kmers
    order = api.length_order(real_batch[2])
    pkw = dict(window_size=ws, **extra)
    want = oracle(oset, real_batch, pkw)
    got, launches, _ = score(ctx, ks, real_batch, pkw, order)
    _cases.same(got, want, ("real length", ws, sorted(extra)))
    assert launches > 0, "the cooperative path did not run"
    if extra:
        co, cr = want["child_offsets"].astype(np.int64), want["child_ranges"]
        assert (co[1:5] - co[:4] > 8).all(), "the long reads are meant to have more than 8 children"
        assert (cr[:, 1] - cr[:, 0]).max() >= 1 << 18, "one child is meant to be long itself"
    pkw2 = dict(pkw, min_mean_q=float(want["mean_q"][1]), min_window_q=float(want["window_q"][2]), max_length=3_000_000)
    want2 = cut_offs(want, real_batch[2], pkw2)
    assert 0 < want2["passed"][:4].sum() < 4
    got2, launches, _ = score(ctx, ks, real_batch, pkw2, order)
    _cases.same(got2, want2, ("real length, cut-offs", ws, sorted(extra)))
    assert launches > 0


# ------------------------------------------------------------------------------------------------------------ 2. engineered coverage
@pytest.fixture(scope="module")
def engineered_batch(kmers):
    ref = kmers[0]
    rng = np.random.default_rng(11)

    def clean(L):
        s = int(rng.integers(0, len(ref) - max(L, 1)))
        return ref[s:s + L].copy()

    reads = []
    for k, (a, b) in enumerate(PERIODS * 2):  # clean / junk periods: the window count hovers on the regimes' edges
        L = int(rng.integers(2000, 9000))
        seq = clean(L)
        pos = int(rng.integers(0, a + b))
        while pos < L:
            pos += a
            e = min(L, pos + b)
            if pos < L:
                seq[pos:e] = junk(rng, e - pos)
            pos = e
        if k >= len(PERIODS):
            sub = rng.random(L) < 0.02
            seq[sub] = junk(rng, int(sub.sum()))
        reads.append(seq.tobytes())
    for ws in (250, 500, 128, 64):
        reads += [clean(L).tobytes() for L in (ws - 1, ws, ws + 1)]
    for L in (1023, 1024, 1025, 2047, 2048, 2049, 32 * 1024 - 1, 32 * 1024, 32 * 1024 + 1):
        seq = clean(L)
        seq[L // 3:L // 3 + 200] = junk(rng, 200)
        reads.append(seq.tobytes())
    reads.append(low(5000).tobytes())         # no coverage: first = -1
    reads.append(clean(6000).tobytes())       # fully covered
    reads.append(b"")
    reads.append(clean(15).tobytes())
    seq = low(4000)                           # covered only in its first 16 and last 16 bases
    seq[:16] = clean(16)
    seq[-16:] = clean(16)
    reads.append(seq.tobytes())
    return api.pack_reads(reads)


@pytest.mark.parametrize("ws,runs", [(250, True), (500, True), (128, True), (64, True), (1000, False), (31, False), (7, False)])
def test_engineered_coverage_through_the_path(ctx, kmers, engineered_batch, ws, runs):
    """FLX_KMER_LONG_MIN=1000: engineered coverage through the path where the window size has a paying regime, through the one-lane
    kernels where it has none; and the same bits with FLX_KMER_FOLD_GRID=0, which keeps the path out."""
    _ref, oset, ks = kmers
    lengths = engineered_batch[2]
    assert (lengths >= 1000).sum() > 40 and (lengths < 1000).sum() > 10
    order = api.length_order(lengths)
    for extra in (dict(), dict(trim=True, split=max(32, ws // 2))):
        pkw = dict(window_size=ws, **extra)
        want = oracle(oset, engineered_batch, pkw)
        got, launches, _ = score(ctx, ks, engineered_batch, pkw, order, {"FLX_KMER_LONG_MIN": "1000"})
        _cases.same(got, want, ("engineered", ws, sorted(extra)))
        assert (launches > 0) == runs, (ws, launches)
        assert want["first"][lengths == 5000][0] == -1
        fp, launches, _ = score(ctx, ks, engineered_batch, pkw, order, {"FLX_KMER_LONG_MIN": "1000", "FLX_KMER_FOLD_GRID": "0"})
        _cases.same(fp, want, ("engineered, FP kernels", ws, sorted(extra)))
        assert launches == 0


# ------------------------------------------------------------------------------------------------------------ 3. skip inside a wave
@pytest.mark.parametrize("extra", [dict(), dict(trim=True, split=100)], ids=["plain", "children"])
def test_skip_inside_a_wave(ctx, kmers, extra):
    """Long and short reads interleaved (130 reads: two full waves and a tail), in file, random and descending order: every output
    of every read equals the run with the path off, bit for bit; then a batch in which every read is long."""
    ref, _oset, ks = kmers
    rng = np.random.default_rng(5)
    lens = [int(rng.integers(1000, 6000)) if i % 3 == 0 else int(rng.integers(1, 1000)) for i in range(64)]
    lens += [int(x) for x in rng.integers(1000, 5000, 64)] + [500, 37]
    reads = []
    for L in lens:
        s = int(rng.integers(0, len(ref) - L))
        seq = ref[s:s + L].copy()
        for _ in range(L // 900):
            n = int(rng.integers(20, 300))
            p = int(rng.integers(0, L - n))
            seq[p:p + n] = junk(rng, n)
        reads.append(seq.tobytes())
    packed = api.pack_reads(reads)
    pkw = dict(window_size=250, min_window_q=50.0, **extra)
    off, launches, _ = score(ctx, ks, packed, pkw, None, {"FLX_KMER_LONG_MIN": "0"})
    assert launches == 0
    for name, order in orders(packed[2]).items():
        got, launches, _ = score(ctx, ks, packed, pkw, order, {"FLX_KMER_LONG_MIN": "1000"})
        _cases.same(got, off, ("mixed waves", name))
        assert launches > 0
    every = api.pack_reads([r for r in reads if len(r) >= 1000])
    off, _, _ = score(ctx, ks, every, pkw, None, {"FLX_KMER_LONG_MIN": "0"})
    for name, order in orders(every[2]).items():
        got, launches, _ = score(ctx, ks, every, pkw, order, {"FLX_KMER_LONG_MIN": "1000"})
        _cases.same(got, off, ("every read long", name))
        assert launches > 0


# ------------------------------------------------------------------------------------------------------------ 4. children at the threshold
def pieces_read(ref, rng, piece_lens, gap):
    """Clean pieces of the given lengths between junk blocks of `gap` bases whose first and last base differ from the reference's
    continuation (so that no 16-mer reaches over a piece's end): the children are the pieces."""
    out = [low(gap)]
    for n in piece_lens:
        s = int(rng.integers(1, len(ref) - n - 1))
        j = low(gap)
        out[-1][-1] = ACGT[(int(np.searchsorted(ACGT, ref[s - 1])) + 1) % 4]
        j[0] = ACGT[(int(np.searchsorted(ACGT, ref[s + n])) + 1) % 4]
        out += [ref[s:s + n].copy(), j]
    return np.concatenate(out).tobytes()


def test_children_at_the_threshold(ctx, kmers):
    """FLX_KMER_LONG_MIN=3000: children of 2999, 3000 and 3001 bases; a long parent with 30 children among short reads with at most
    8 does not launch MODE 5, one short read with 9 children does, and the results stay equal to the oracle."""
    ref, oset, ks = kmers
    rng = np.random.default_rng(9)
    N = 3000
    long_parent = pieces_read(ref, rng, [N - 1, N, N + 1] + [int(x) for x in rng.integers(100, 2500, 27)], 150)
    short = [pieces_read(ref, rng, [int(x) for x in rng.integers(100, 180, k)], 150) for k in (1, 2, 5, 8, 8, 3)]
    short += [ref[1000:1000 + int(L)].tobytes() for L in rng.integers(50, 2900, 60)]
    assert all(len(r) < N for r in short)
    pkw = dict(window_size=250, trim=True, split=100)
    env = {"FLX_KMER_LONG_MIN": str(N)}
    packed = api.pack_reads([long_parent] + short)
    want = oracle(oset, packed, pkw)
    co = want["child_offsets"].astype(np.int64)
    child_len = want["child_ranges"][:, 1] - want["child_ranges"][:, 0]
    assert co[1] - co[0] == 30 and (co[2:] - co[1:-1]).max() == 8
    assert {N - 1, N, N + 1} <= set(int(x) for x in child_len[:30])
    got, launches, m5 = score(ctx, ks, packed, pkw, api.length_order(packed[2]), env)
    _cases.same(got, want, "long parent with 30 children")
    assert launches > 0 and m5 == 0
    nine = pieces_read(ref, rng, [150] * 9, 150)
    assert len(nine) < N
    packed = api.pack_reads([long_parent] + short + [nine])
    want = oracle(oset, packed, pkw)
    co = want["child_offsets"].astype(np.int64)
    assert co[-1] - co[-2] == 9
    got, launches, m5 = score(ctx, ks, packed, pkw, api.length_order(packed[2]), env)
    _cases.same(got, want, "and a short read with 9 children")
    assert launches > 0 and m5 > 0


# ------------------------------------------------------------------------------------------------------------ 5. where the path stays out
@pytest.mark.parametrize("pkw,env", [(dict(trim=True, split=16), {}), (dict(trim=True, split=100), {"FLX_KMER_FOLD": "words"}),
                                     (dict(trim=True, split=100), {"FLX_KMER_FOLD": "bits"}), (dict(), {"FLX_KMER_FOLD_EVENTS": "1"}),
                                     (dict(trim=True, split=100), {"FLX_KMER_FOLD_EVENTS": "1"})],
                         ids=["split16", "words", "bits", "events", "events+children"])
def test_the_path_stays_out(ctx, kmers, engineered_batch, pkw, env):
    _ref, oset, ks = kmers
    want = oracle(oset, engineered_batch, pkw)
    got, launches, _ = score(ctx, ks, engineered_batch, pkw, api.length_order(engineered_batch[2]), dict(env, FLX_KMER_LONG_MIN="1000"))
    _cases.same(got, want, ("stays out", sorted(env)))
    assert launches == 0


def test_ordinary_batch_does_not_take_the_path(ctx, kmers):
    """Reads of up to 200 kbp at the default threshold: nothing but the count runs."""
    ref, oset, ks = kmers
    rng = np.random.default_rng(21)
    reads = []
    for L in [200_000, 150_000] + [int(x) for x in rng.integers(100, 30_000, 300)]:
        s = int(rng.integers(0, len(ref) - L))
        seq = ref[s:s + L].copy()
        seq[L // 2:L // 2 + 40] = junk(rng, 40)
        reads.append(seq.tobytes())
    packed = api.pack_reads(reads)
    for pkw in (dict(), dict(trim=True, split=500)):
        got, launches, _ = score(ctx, ks, packed, pkw, api.length_order(packed[2]))
        _cases.same(got, oracle(oset, packed, pkw), "ordinary batch")
        assert launches == 0


# ------------------------------------------------------------------------------------------------------------ 6. the switch
@pytest.mark.parametrize("value", ["-1", "abc", "1k"])
def test_switch_rejects_bad_values(ctx, kmers, value):
    ref, _oset, ks = kmers
    packed = api.pack_reads([ref[:3000].tobytes()])
    with pytest.raises(api.FlxError, match="FLX_KMER_LONG_MIN"):
        score(ctx, ks, packed, dict(), None, {"FLX_KMER_LONG_MIN": value})


def test_switch_zero_turns_the_path_off(ctx, kmers):
    ref, oset, ks = kmers
    packed = api.pack_reads([ref[:300_000].tobytes(), ref[5000:9000].tobytes()])
    want = oracle(oset, packed, dict())
    got, launches, _ = score(ctx, ks, packed, dict())
    _cases.same(got, want, "default")
    assert launches > 0
    got, launches, _ = score(ctx, ks, packed, dict(), None, {"FLX_KMER_LONG_MIN": "0"})
    _cases.same(got, want, "off")
    assert launches == 0


# ------------------------------------------------------------------------------------------------------------ 7. one 4 Mbp read
@pytest.mark.parametrize("children", [False, True], ids=["plain", "trim+split500"])
def test_one_4mbp_read_is_fast(ctx, kmers, children):
    """One 4 Mbp read, device-resident, window 250, plain and with --trim --split 500 (a long child): the cooperative folds
    (flx_score_kmer_long) take at most a quarter of the one-lane folds' time (flx_score_kmer_fold with FLX_KMER_LONG_MIN=0), same bits.
    The factor is the Phred test's: a guard against a silently serial path, not a target.  The test prints both times."""
    import torch
    from filtlong_amd import _lib
    ref, _oset, ks = kmers
    rng = np.random.default_rng(77)
    L = 4_000_000
    seq = tiled(ref, rng, L)
    sub = rng.random(L) < 0.03
    seq[sub] = junk(rng, int(sub.sum()))
    for p in rng.integers(1000, L - 400_000, 40):
        n = int(rng.choice([40, 300, 600, 3000]))
        seq[p:p + n] = junk(rng, n)
    seq[:300] = junk(rng, 300)
    seq[-300:] = junk(rng, 300)
    plane, offsets, lengths = api.pack_reads([seq.tobytes()])
    d_plane = torch.from_numpy(plane).cuda()
    d_off = torch.from_numpy(offsets.view(np.int64)).cuda()
    d_len = torch.from_numpy(lengths).cuda()
    cap = 4096
    t = {k: torch.zeros(sz, dtype=dt, device="cuda") for k, sz, dt in (
        ("mean", 1, torch.float64), ("win", 1, torch.float64), ("pass", 1, torch.uint8), ("first", 1, torch.int32), ("last", 1, torch.int32),
        ("coff", 2, torch.int64), ("crng", 2 * cap, torch.int32), ("cmean", cap, torch.float64), ("cwin", cap, torch.float64),
        ("cpass", cap, torch.uint8))}
    s = _lib.Scores()
    s.mean_q, s.window_q, s.passed, s.first, s.last = (t["mean"].data_ptr(), t["win"].data_ptr(), t["pass"].data_ptr(),
                                                      t["first"].data_ptr(), t["last"].data_ptr())
    s.child_offsets, s.child_ranges, s.child_mean_q, s.child_window_q, s.child_passed = (
        t["coff"].data_ptr(), t["crng"].data_ptr(), t["cmean"].data_ptr(), t["cwin"].data_ptr(), t["cpass"].data_ptr())
    s.child_capacity = cap
    params = api.make_params(window_size=250, trim=children, split=500 if children else None)

    def timed(reps, prefix, budget_s):
        ms = []
        t0 = time.perf_counter()
        for _ in range(reps):
            ctx.timing_enable(True)
            ctx.timing_reset()
            ctx.score_kmer_dev(ks, d_plane.data_ptr(), plane.nbytes, d_off.data_ptr(), d_len.data_ptr(), None, 1, params, s)
            torch.cuda.synchronize()
            ms.append(ctx.timing_get(prefix)[0])
            ctx.timing_enable(False)
            assert time.perf_counter() - t0 < budget_s, "a scoring call of one read takes far longer than it should"
        nc = int(s.n_children)
        res = [t[k].cpu().numpy().copy() for k in ("mean", "win", "pass", "first", "last")] + \
              [t["crng"][:2 * nc].cpu().numpy().copy(), t["cmean"][:nc].cpu().numpy().view(np.uint64).copy(),
               t["cwin"][:nc].cpu().numpy().view(np.uint64).copy(), t["cpass"][:nc].cpu().numpy().copy()]
        return float(np.median(ms[1:])), res

    with pytest.MonkeyPatch.context() as mp:
        mp.delenv("FLX_KMER_LONG_MIN", raising=False)
        fast, r_fast = timed(5, "flx_score_kmer_long", 10.0)
        mp.setenv("FLX_KMER_LONG_MIN", "0")
        slow, r_slow = timed(3, "flx_score_kmer_fold", 3 * 0.5 + 10.0)  # (about 0.5 s per call would already be five times the estimate)
    print("4 Mbp read (%s): cooperative folds %.3f ms, one-lane folds %.3f ms, %d children" % ("trim + split 500" if children else "plain", fast, slow, int(s.n_children)))
    for a, b in zip(r_fast, r_slow):
        assert a.shape == b.shape and (a.view(np.uint8) == b.view(np.uint8)).all()
    if children:
        assert (r_fast[5].reshape(-1, 2)[:, 1] - r_fast[5].reshape(-1, 2)[:, 0]).max() >= 1 << 18, "a child is meant to be long itself"
    assert fast > 0.0 and fast <= 0.25 * slow, (fast, slow)


# ------------------------------------------------------------------------------------------------------------ 8. command line
def test_end_to_end_against_the_reference_binary(tmp_path, kmers):
    """One 300 kbp and one 1 Mbp read among 2000 ordinary ones, `-a assembly --trim --split 500 --min_length 1000`: one process, then
    two forked ranks over the loopback communicator — stdout byte-identical to the reference binary's."""
    if not os.path.exists(_oracle.REF_FILTLONG):
        pytest.skip("reference binary not built")
    ref = kmers[0]
    rng = np.random.default_rng(31)
    lens = [int(x) for x in rng.integers(300, 12_000, 2000)] + [300_000, 1_000_000]
    recs = []
    for j, i in enumerate(rng.permutation(len(lens))):
        L = lens[i]
        seq = tiled(ref, rng, L) if L > 200_000 else ref[int(rng.integers(0, len(ref) - L)):][:L].copy()
        sub = rng.random(L) < 0.03
        seq[sub] = junk(rng, int(sub.sum()))
        for _ in range(L // 40_000 + (1 if L > 3000 and j % 2 else 0)):
            n = int(rng.choice([60, 600, 1500]))
            p = int(rng.integers(0, L - n))
            seq[p:p + n] = junk(rng, n)
        recs.append(b"@r%d\n%s\n+\n%s\n" % (j, seq.tobytes(), S.qual_read(j, L).tobytes()))
    fq, fa = tmp_path / "reads.fastq", tmp_path / "asm.fasta"
    fq.write_bytes(b"".join(recs))
    fa.write_bytes(_cases.fasta_bytes([ref.tobytes()]))
    args = ["-a", str(fa), "--trim", "--split", "500", "--min_length", "1000", str(fq)]
    env = dict(os.environ, LANG="C", LC_ALL="C")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK") + SWITCHES:
        env.pop(k, None)
    want = subprocess.run([_oracle.REF_FILTLONG] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
    assert want.returncode == 0 and len(want.stdout) > 0
    new = subprocess.run([BIN] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(env, FLX_API_TIMING="1"))
    assert new.returncode == 0, new.stderr[-500:]
    assert new.stdout == want.stdout
    assert b"kmer long reads" in new.stderr  # the cooperative path ran (FLX_API_TIMING stage line)
    shim_dir = os.path.join(ROOT, "tests", "shim")
    subprocess.check_call(["make", "-s", "-C", shim_dir])
    env2 = dict(env, FLX_RCCL_LIB=os.path.join(shim_dir, "libloopback_rccl.so"), FLX_DEVICE="0")
    new2 = subprocess.run([BIN, "--gpus", "2"] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env2)
    assert new2.returncode == 0, new2.stderr[-500:]
    assert new2.stdout == want.stdout
