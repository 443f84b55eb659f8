"""k-mer mode: the coverage of ultra-long reads in segments, one wave each (csrc/cover_long.hip, csrc/cover_segments.h) —
bit-identical to the oracle and the reference binary.

Reads from a length threshold on (2^18 bases, raised with the batch's bases per resident wave; FLX_KMER_COVER_LONG_MIN=N forces N, 0
turns the path off) are left alone by the batch launch of k_kmer_cover_q / k_kmer_cover_w and covered as segments of
FLX_KMER_COVER_LONG_SPANS spans — virtual reads with 32 bases of context, of which only the owned bases are written and counted —
by the same kernels.  Whether the path ran is visible in flx_timing_get under "flx_score_kmer_cover.long".  Unless a test says
otherwise it forces FLX_KMER_COVER_LONG_MIN=2048 and keeps the cooperative folds out (FLX_KMER_LONG_MIN=0)."""
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
SWITCHES = ("FLX_KMER_COVER_LONG_MIN", "FLX_KMER_COVER_LONG_SPANS", "FLX_KMER_LONG_MIN", "FLX_KMER_COVER", "FLX_KMER_LOCUS", "FLX_KMER_PAIRTABLE",
            "FLX_KMER_FOLD", "FLX_KMER_FOLD_GRID", "FLX_KMER_FOLD_EVENTS")
FORCED = {"FLX_KMER_COVER_LONG_MIN": "2048", "FLX_KMER_LONG_MIN": "0"}
BRACKET = "flx_score_kmer_cover.long"


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def kmers(ctx):
    """The reference set of tests/test_gpu_kmer_long.py: (reference bases, oracle set, device set)."""
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
    """n bases with three distinct 16-mers, none of them in the set."""
    return np.frombuffer((b"ACG" * (n // 3 + 1))[:n], dtype=np.uint8).copy()


def tiled(ref, rng, L):
    out = []
    while sum(len(x) for x in out) < L:
        n = int(rng.integers(20_000, 150_000))
        s = int(rng.integers(0, len(ref) - n))
        out.append(ref[s:s + n])
    return np.concatenate(out)[:L].copy()


def cap(lengths):
    return max(64, len(lengths)) * 40


def score(ctx, ks, packed, pkw, order=None, env=None, defaults=FORCED):
    """One scoring call under `defaults` and `env` (every other switch unset): (scores, launches of the cover path's bracket)."""
    plane, offsets, lengths = packed
    with pytest.MonkeyPatch.context() as mp:
        for k in SWITCHES:
            mp.delenv(k, raising=False)
        for k, v in dict(defaults, **(env or {})).items():
            if v is not None:
                mp.setenv(k, v)
        ctx.timing_enable(True)
        ctx.timing_reset()
        try:
            got = ctx.score_reads(plane, offsets, lengths, api.make_params(**pkw), kmers=ks, order=order, child_capacity=cap(lengths))
            return got, ctx.timing_get(BRACKET)[1]
        finally:
            ctx.timing_enable(False)


def oracle(oset, packed, pkw):
    plane, offsets, lengths = packed
    return _oracle.score_plane_mt(plane, offsets, lengths, _oracle.make_params(**pkw), kmerset=oset, child_cap=cap(lengths))


def orders(lengths, seed=3):
    return {None: None, "random": np.random.default_rng(seed).permutation(len(lengths)).astype(np.uint32), "desc": api.length_order(lengths)}


# ------------------------------------------------------------------------------------------------------------ 1. islands across boundaries
@pytest.mark.parametrize("P", [1, 2])
def test_islands_across_segment_boundaries(ctx, kmers, P):
    """Reads of 4 P 1024 + 37 bases of non-member background with one clean island of 16 .. 64 bases that starts at boundary + d, d =
    -70 .. +40, at the first and the last segment boundary; window 32, --trim --split 32.  Every field equals the oracle's and the run
    with the path off, and the path ran."""
    ref, oset, ks = kmers
    rng = np.random.default_rng(100 + P)
    L = 4 * P * 1024 + 37
    reads = []
    for boundary in (P * 1024, 4 * P * 1024):
        for island in (16, 17, 31, 32, 33, 48, 64):
            for d in range(-70, 41):
                seq = low(L)
                at = boundary + d
                n = max(0, min(island, L - at))  # (behind the last boundary the read has 37 bases: the island ends with the read)
                s = int(rng.integers(0, len(ref) - island))
                seq[at:at + n] = ref[s:s + n]
                reads.append(seq.tobytes())
    packed = api.pack_reads(reads)
    pkw = dict(window_size=32, trim=True, split=32)
    env = {"FLX_KMER_COVER_LONG_SPANS": str(P)}
    want = oracle(oset, packed, pkw)
    assert (want["first"] >= 0).sum() > len(reads) * 0.8
    got, launches = score(ctx, ks, packed, pkw, None, env)
    _cases.same(got, want, ("islands", P))
    assert launches > 0, "the cover path did not run"
    off, launches = score(ctx, ks, packed, pkw, None, dict(env, FLX_KMER_COVER_LONG_MIN="0"))
    _cases.same(got, off, ("islands, path off", P))
    assert launches == 0


# ------------------------------------------------------------------------------------------------------------ 2. lengths on the edges
THR = 2048
EDGES = (-33, -32, -31, -17, -16, -15, -1, 0, 1, 15, 16, 17, 31, 32, 33)


@pytest.fixture(scope="module")
def edge_batch(kmers):
    """Reads with 3 % substitutions: thr - 1 .. thr + 1, k P 1024 + e around the segment boundaries of P = 1 and P = 3, a last segment of
    1 .. 33 bases, a fully covered read, a read without coverage and a read covered only in its first and last 16 bases."""
    ref = kmers[0]
    rng = np.random.default_rng(41)
    lens = [THR - 1, THR, THR + 1]
    for P in (1, 3):
        for k in (2, 3) if P == 1 else (1, 2):
            lens += [k * P * 1024 + e for e in EDGES]
        lens += [3 * P * 1024 + t for t in range(1, 34)]
    reads = []
    for L in lens:
        s = int(rng.integers(0, len(ref) - L))
        seq = ref[s:s + L].copy()
        sub = rng.random(L) < 0.03
        seq[sub] = junk(rng, int(sub.sum()))
        reads.append(seq.tobytes())
    reads.append(ref[1000:1000 + 7000].tobytes())  # fully covered
    reads.append(low(7001).tobytes())              # no coverage: first = last = -1
    seq = low(6200)
    seq[:16] = ref[5000:5016]
    seq[-16:] = ref[9000:9016]
    reads.append(seq.tobytes())
    reads += [ref[20_000:20_000 + int(L)].tobytes() for L in rng.integers(1, 2000, 40)]  # short reads between them
    return api.pack_reads(reads)


@pytest.fixture(scope="module")
def edge_want(kmers, edge_batch):
    return {name: oracle(kmers[1], edge_batch, pkw) for name, pkw in (("plain", dict()), ("children", dict(trim=True, split=100)))}


@pytest.mark.parametrize("form,runs", [({}, True), ({"FLX_KMER_COVER": "q2"}, True), ({"FLX_KMER_COVER": "w"}, True), ({"FLX_KMER_LOCUS": "0"}, True),
                                       ({"FLX_KMER_COVER": "v2"}, False), ({"FLX_KMER_PAIRTABLE": "0"}, False)],
                         ids=["default", "q2", "w", "locus0", "v2", "pairtable0"])
@pytest.mark.parametrize("P", [1, 3])
def test_lengths_on_the_edges(ctx, kmers, edge_batch, edge_want, form, runs, P):
    """Every coverage form, processing orders None / random / descending: every field equals the oracle's.  k_kmer_cover (v2) and a set
    without a pair table keep long reads in their own launch: the bracket does not appear and the bits are the same."""
    ref, _oset, ks = kmers
    own = None
    if "FLX_KMER_PAIRTABLE" in form:  # (the switch is read when a set is finalized)
        with pytest.MonkeyPatch.context() as mp:
            mp.setenv("FLX_KMER_PAIRTABLE", "0")
            own = api.Kmers(ctx)
            own.add_assembly_fasta([ref.tobytes()])
            own.finalize()
    try:
        want = edge_want["plain"]
        assert want["first"][edge_batch[2] == 7001][0] == -1 and want["first"][edge_batch[2] == 6200][0] == 0
        for name, pkw in (("plain", dict()), ("children", dict(trim=True, split=100))):
            for oname, order in orders(edge_batch[2]).items():
                got, launches = score(ctx, own or ks, edge_batch, pkw, order, dict(form, FLX_KMER_COVER_LONG_SPANS=str(P)))
                _cases.same(got, edge_want[name], ("edges", sorted(form), P, name, oname))
                assert (launches > 0) == runs, (sorted(form), launches)
    finally:
        if own is not None:
            own.close()


# ------------------------------------------------------------------------------------------------------------ 3. indels per segment
def with_indels(rng, seq):
    """An insertion or a deletion of 1-3 bases every 12-25 bases."""
    out, p = [], 0
    while p < len(seq):
        n = int(rng.integers(12, 26))
        out.append(seq[p:p + n])
        p += n
        k = int(rng.integers(1, 4))
        if rng.random() < 0.5:
            out.append(junk(rng, k))
        else:
            p += k
    return np.concatenate(out)


@pytest.mark.parametrize("form", [{}, {"FLX_KMER_COVER": "q2"}], ids=["default", "q2"])
@pytest.mark.parametrize("P", [1, 2])
def test_indels_per_segment(ctx, form, P):
    """Reads of 8-20 kbp whose alternate segments carry an insertion or deletion every 12-25 bases, the others clean; both strands, and
    a read that changes contig at a segment boundary (the 400 kbp reference as two contigs).  Parity with the oracle only: how many
    segments the first kernel hands to the lane-diagonal kernel is its own business."""
    ref = S.bases_read(S.STREAM_REF, 0, 0, 400_000)
    contigs = [ref[:200_000].tobytes(), ref[200_000:].tobytes()]
    oset = _oracle.KmerSet()
    oset.add_assembly(contigs)
    ks = api.Kmers(ctx)
    ks.add_assembly_fasta(contigs)
    ks.finalize()
    try:
        rng = np.random.default_rng(7 + P)
        seg = P * 1024
        reads = []
        for i in range(24):
            L = int(rng.integers(8000, 20_000))
            parts, k = [], 0
            s = int(rng.integers(0, 200_000 - 2 * L))
            while sum(len(x) for x in parts) < L:
                piece = ref[s:s + seg]
                s += seg
                if i == 0 and k == 3:  # the read goes on in the other contig from this boundary on
                    s = 200_000 + int(rng.integers(0, 200_000 - 2 * L))
                    piece = ref[s:s + seg]
                    s += seg
                if k % 2 == (i & 1):
                    piece = with_indels(rng, piece)[:seg]
                    piece = np.concatenate([piece, junk(rng, seg - len(piece))])
                parts.append(piece)
                k += 1
            seq = np.concatenate(parts)[:L]
            raw = seq.tobytes()
            reads.append(_cases.revcomp(raw) if i % 3 == 1 else raw)
        packed = api.pack_reads(reads)
        for pkw in (dict(), dict(trim=True, split=100)):
            want = oracle(oset, packed, pkw)
            got, launches = score(ctx, ks, packed, pkw, api.length_order(packed[2]), dict(form, FLX_KMER_COVER_LONG_SPANS=str(P)))
            _cases.same(got, want, ("indels", sorted(form), P, sorted(pkw)))
            assert launches > 0
    finally:
        ks.close()


# ------------------------------------------------------------------------------------------------------------ 4. real length, default switches
@pytest.fixture(scope="module")
def real_batch(kmers):
    """One read of 300 kbp and one of 1 Mbp tiled from the reference with 3 % substitutions and junk blocks among 200 short reads."""
    ref = kmers[0]
    rng = np.random.default_rng(2025)
    reads = []
    for L in (300_000, 1_000_000):
        seq = tiled(ref, rng, L)
        sub = rng.random(L) < 0.03
        seq[sub] = junk(rng, int(sub.sum()))
        for _ in range(30 + L // 100_000):
            n = int(rng.choice([20, 40, 70, 300, 600, 2000, 5000]))
            p = int(rng.integers(0, L - n))
            seq[p:p + n] = junk(rng, n)
        head, tail = int(rng.integers(30, 900)), int(rng.integers(30, 900))
        seq[:head] = junk(rng, head)
        seq[L - tail:] = junk(rng, tail)
        reads.append(seq.tobytes())
    for L in rng.integers(1, 20_000, 200):
        s = int(rng.integers(0, len(ref) - int(L)))
        seq = ref[s:s + int(L)].copy()
        sub = rng.random(int(L)) < 0.05
        seq[sub] = junk(rng, int(sub.sum()))
        reads.append(seq.tobytes())
    return api.pack_reads(reads)


@pytest.mark.parametrize("extra", [dict(), dict(trim=True, split=500)], ids=["plain", "trim+split500"])
@pytest.mark.parametrize("ws", [250, 1000])
def test_parity_at_real_length(ctx, kmers, real_batch, ws, extra):
    """Default threshold and segment size.  Window 1000 has no paying fold regime: only the cover path is cooperative there.  First
    with the cooperative folds off, then with them on as well (FLX_KMER_LONG_MIN unset)."""
    _ref, oset, ks = kmers
    order = api.length_order(real_batch[2])
    pkw = dict(window_size=ws, **extra)
    want = oracle(oset, real_batch, pkw)
    got, launches = score(ctx, ks, real_batch, pkw, order, None, {"FLX_KMER_LONG_MIN": "0"})
    _cases.same(got, want, ("real length, folds off", ws, sorted(extra)))
    assert launches > 0, "the cover path did not run"
    got, launches = score(ctx, ks, real_batch, pkw, order, None, {})
    _cases.same(got, want, ("real length, folds on", ws, sorted(extra)))
    assert launches > 0


# ------------------------------------------------------------------------------------------------------------ 5. the switches
@pytest.mark.parametrize("name", ["FLX_KMER_COVER_LONG_MIN", "FLX_KMER_COVER_LONG_SPANS"])
@pytest.mark.parametrize("value", ["-1", "abc", "1k", ""])
def test_switches_reject_bad_values(ctx, kmers, name, value):
    ref, _oset, ks = kmers
    packed = api.pack_reads([ref[:3000].tobytes()])
    with pytest.raises(api.FlxError, match=name):
        score(ctx, ks, packed, dict(), None, {name: value})


def test_zero_spans_is_rejected(ctx, kmers):
    ref, _oset, ks = kmers
    with pytest.raises(api.FlxError, match="FLX_KMER_COVER_LONG_SPANS"):
        score(ctx, ks, api.pack_reads([ref[:3000].tobytes()]), dict(), None, {"FLX_KMER_COVER_LONG_SPANS": "0"})


def test_zero_turns_the_path_off_and_short_batches_stay_out(ctx, kmers):
    ref, oset, ks = kmers
    packed = api.pack_reads([ref[:9000].tobytes(), ref[5000:7047].tobytes(), ref[100:1100].tobytes()])
    want = oracle(oset, packed, dict())
    got, launches = score(ctx, ks, packed, dict())
    _cases.same(got, want, "forced")
    assert launches > 0
    got, launches = score(ctx, ks, packed, dict(), None, {"FLX_KMER_COVER_LONG_MIN": "0"})
    _cases.same(got, want, "off")
    assert launches == 0
    short = api.pack_reads([ref[5000:7047].tobytes(), ref[100:1100].tobytes()])  # the longest read is one base short of the threshold
    got, launches = score(ctx, ks, short, dict())
    _cases.same(got, oracle(oset, short, dict()), "no read at the threshold")
    assert launches == 0
    got, launches = score(ctx, ks, packed, dict(), None, None, {})  # default threshold: 2^18 bases
    _cases.same(got, want, "default threshold")
    assert launches == 0


# ------------------------------------------------------------------------------------------------------------ 6. command line
def test_end_to_end_against_the_reference_binary(tmp_path, kmers):
    """Reads of 5-30 kbp, `-a assembly --trim --split 500 --keep_percent 80`, forced switches (threshold 2048, P = 2) through the streamed
    ingest in small chunks: exit code, stdout bytes and raw stderr of the reference binary."""
    if not os.path.exists(_oracle.REF_FILTLONG):
        pytest.skip("reference binary not built")
    ref = kmers[0]
    rng = np.random.default_rng(33)
    recs = []
    for j in range(120):
        L = int(rng.integers(5000, 30_000))
        seq = ref[int(rng.integers(0, len(ref) - L)):][:L].copy()
        sub = rng.random(L) < 0.03
        seq[sub] = junk(rng, int(sub.sum()))
        for _ in range(j % 3):
            n = int(rng.choice([60, 600, 1500]))
            p = int(rng.integers(0, L - n))
            seq[p:p + n] = junk(rng, n)
        recs.append(b"@r%d\n%s\n+\n%s\n" % (j, seq.tobytes(), S.qual_read(j, L).tobytes()))
    fq, fa = tmp_path / "reads.fastq", tmp_path / "asm.fasta"
    fq.write_bytes(b"".join(recs))
    fa.write_bytes(_cases.fasta_bytes([ref.tobytes()]))
    args = ["-a", str(fa), "--trim", "--split", "500", "--keep_percent", "80", str(fq)]
    env = dict(os.environ, LANG="C", LC_ALL="C")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK") + SWITCHES:
        env.pop(k, None)
    want = subprocess.run([_oracle.REF_FILTLONG] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
    assert want.returncode == 0 and len(want.stdout) > 0
    forced = dict(env, FLX_KMER_COVER_LONG_MIN="2048", FLX_KMER_COVER_LONG_SPANS="2", FLX_CLI_FORCE_STREAM="1", FLX_CLI_CHUNK_BYTES="200000",
                  FLX_CLI_BLOCK_BYTES="65536")
    new = subprocess.run([BIN] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=forced)
    assert (new.returncode, new.stderr) == (want.returncode, want.stderr), new.stderr[-500:]
    assert new.stdout == want.stdout
    timed = subprocess.run([BIN] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(forced, FLX_API_TIMING="1"))
    assert timed.returncode == 0 and timed.stdout == want.stdout
    assert b"kmer long cover" in timed.stderr  # the path ran in the command line (FLX_API_TIMING stage line)


# ------------------------------------------------------------------------------------------------------------ 7. guard against serialisation
def test_one_4mbp_read_is_not_serial(ctx, kmers):
    """One 4 Mbp read alone, device-resident, default switches: the cover stage (flx_score_kmer_cover, both brackets) with the path on
    takes at most a quarter of its time with FLX_KMER_COVER_LONG_MIN=0, same bits.  At 32 spans the read is 123 segments, so anything
    above a quarter means the segments do not run concurrently: a guard, not the performance claim.  The test prints both times."""
    import torch
    from filtlong_amd import _lib
    ref, _oset, ks = kmers
    rng = np.random.default_rng(78)
    L = 4_000_000
    seq = tiled(ref, rng, L)
    sub = rng.random(L) < 0.03
    seq[sub] = junk(rng, int(sub.sum()))
    for p in rng.integers(1000, L - 400_000, 40):
        n = int(rng.choice([40, 300, 600, 3000]))
        seq[p:p + n] = junk(rng, n)
    plane, offsets, lengths = api.pack_reads([seq.tobytes()])
    d_plane = torch.from_numpy(plane).cuda()
    d_off = torch.from_numpy(offsets.view(np.int64)).cuda()
    d_len = torch.from_numpy(lengths).cuda()
    t = {k: torch.zeros(sz, dtype=dt, device="cuda") for k, sz, dt in (
        ("mean", 1, torch.float64), ("win", 1, torch.float64), ("pass", 1, torch.uint8), ("first", 1, torch.int32), ("last", 1, torch.int32),
        ("coff", 2, torch.int64))}
    s = _lib.Scores()
    s.mean_q, s.window_q, s.passed, s.first, s.last = (t["mean"].data_ptr(), t["win"].data_ptr(), t["pass"].data_ptr(),
                                                      t["first"].data_ptr(), t["last"].data_ptr())
    s.child_offsets = t["coff"].data_ptr()
    params = api.make_params(window_size=250)

    def timed(reps, budget_s):
        ms, n = [], 0
        t0 = time.perf_counter()
        for _ in range(reps):
            ctx.timing_enable(True)
            ctx.timing_reset()
            ctx.score_kmer_dev(ks, d_plane.data_ptr(), plane.nbytes, d_off.data_ptr(), d_len.data_ptr(), None, 1, params, s)
            torch.cuda.synchronize()
            ms.append(ctx.timing_get("flx_score_kmer_cover")[0])
            n = ctx.timing_get(BRACKET)[1]
            ctx.timing_enable(False)
            assert time.perf_counter() - t0 < budget_s, "a scoring call of one read takes far longer than it should"
        return float(np.median(ms[1:])), n, [t[k].cpu().numpy().copy() for k in ("mean", "win", "pass", "first", "last")]

    with pytest.MonkeyPatch.context() as mp:
        for k in SWITCHES:
            mp.delenv(k, raising=False)
        fast, n_fast, r_fast = timed(5, 10.0)
        mp.setenv("FLX_KMER_COVER_LONG_MIN", "0")
        slow, n_slow, r_slow = timed(3, 3 * 0.5 + 10.0)
    print("4 Mbp read: cover stage in segments %.3f ms, one wave %.3f ms" % (fast, slow))
    assert n_fast > 0 and n_slow == 0
    for a, b in zip(r_fast, r_slow):
        assert a.shape == b.shape and (a.view(np.uint8) == b.view(np.uint8)).all()
    assert fast > 0.0 and fast <= 0.25 * slow, (fast, slow)
