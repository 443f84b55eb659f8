"""Phred scoring of very long reads, many lanes per read (score_phred_long.hip) — bit-identical to the oracle and the reference binary.

Reads from a length threshold on (2^18 bases or more, raised with the batch's bases per lane; FLX_PHRED_LONG_MIN=N forces N, 0 turns
the path off) are left alone by the batch kernel and folded cooperatively; the kernel FLX_PHRED_KERNEL selects scores the rest of the batch.
Whether the path ran is visible in flx_timing_get under the prefix "flx_score_phred_long".
"""
import os
import subprocess
import time

import numpy as np
import pytest

import _oracle
from filtlong_amd import api

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "filtlong_amd", "bin", "filtlong")
KERNELS = ["default", "dual", "ring", "stream", "direct"]  # the FLX_PHRED_KERNEL values (default: unset)


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


def ont_qual(L, seed, dips=0.03, centre=(5.0, 3.0)):
    """ONT-like quality string: runs of ~300 bases around a gamma-distributed centre (default Q ~15), per-base noise, and some
    low-quality stretches (Q 0-3: window values around and below 0.5, i.e. binade changes of the window fold)."""
    rng = np.random.default_rng(seed)
    run = 300
    seg = rng.gamma(centre[0], centre[1], L // run + 2).astype(np.float32)
    low = rng.random(len(seg)) < dips
    seg[low] = rng.uniform(0.0, 3.0, int(low.sum()))
    q = np.repeat(seg, run)[:L] + rng.standard_normal(L, dtype=np.float32) * np.float32(4.0)
    return (np.clip(np.rint(q), 0, 60) + 33).astype(np.uint8).tobytes()


def bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64)


def assert_same(got, want, what):
    for key in ("mean_q", "window_q"):
        g, w = np.asarray(got[key], dtype=np.float64), np.asarray(want[key], dtype=np.float64)
        assert (np.isnan(g) == np.isnan(w)).all(), what + " " + key + ": NaN pattern differs"
        bad = np.nonzero((bits(g) != bits(w)) & ~np.isnan(w))[0]
        assert len(bad) == 0, "%s %s: %d of %d differ, first read %d: got %s want %s" % (
            what, key, len(bad), len(w), bad[0], float(g[bad[0]]).hex(), float(w[bad[0]]).hex())
    assert (np.asarray(got["passed"]) == np.asarray(want["passed"])).all(), what + " passed"


def score_both(ctx, quals, pkw, order="desc", want=None):
    plane, offsets, lengths = api.pack_reads(quals)
    if want is None:
        want = _oracle.score_plane_mt(plane, offsets, lengths, _oracle.make_params(**pkw))
    if order == "desc":
        ordr = api.length_order(lengths)
    elif order == "random":
        ordr = np.random.default_rng(len(quals)).permutation(len(quals)).astype(np.uint32)
    else:
        ordr = None
    ctx.timing_enable(True)
    ctx.timing_reset()
    got = ctx.score_reads(plane, offsets, lengths, api.make_params(**pkw), order=ordr)
    launches = ctx.timing_get("flx_score_phred_long")[1]
    ctx.timing_enable(False)
    return got, want, launches


def set_kernel(monkeypatch, kernel):
    if kernel == "default":
        monkeypatch.delenv("FLX_PHRED_KERNEL", raising=False)
    else:
        monkeypatch.setenv("FLX_PHRED_KERNEL", kernel)


@pytest.fixture(scope="module")
def long_reads():
    return [ont_qual(L, 1000 + i) for i, L in enumerate((300_000, 1_000_000, 2_500_000, 4_000_000))]


@pytest.mark.parametrize("ws", [1, 7, 250, 623, 624, 5000, 300_000])
def test_parity_at_real_length(ctx, long_reads, ws, monkeypatch):
    """Reads of 0.3 / 1 / 2.5 / 4 Mbp among ordinary ones, at the threshold chosen from the data: every field bit-identical, with the
    hard cut-offs set to the oracle's exact values."""
    monkeypatch.delenv("FLX_PHRED_LONG_MIN", raising=False)
    short = [ont_qual(int(L), 50 + i) for i, L in enumerate(np.random.default_rng(ws).integers(1, 20_000, 200))]
    quals = long_reads + short
    got, want, launches = score_both(ctx, quals, dict(window_size=ws))
    assert_same(got, want, "ws=%d" % ws)
    assert launches > 0
    pkw = dict(window_size=ws, min_mean_q=float(want["mean_q"][1]), min_window_q=float(want["window_q"][2]), max_length=3_000_000)
    got, want2, launches = score_both(ctx, quals, pkw)
    assert_same(got, want2, "ws=%d cut-offs" % ws)
    assert launches > 0


def adversarial_reads(ws):
    rng = np.random.default_rng(ws + 7)
    reads = [b"!" * 50_000, b"!~" * 25_000]
    # a slow drift of the share of quality-0 bases: the window (and, early on, the mean) crosses the 0.5, 0.25 and 0.125 binades
    x = np.arange(200_000)
    p = 0.5 + 0.5 * np.sin(2 * np.pi * x / 20_000)
    hi = rng.integers(36, 40, len(x))  # Q 3..6: quality values around 0.5
    reads.append(np.where(rng.random(len(x)) < p, 33, hi).astype(np.uint8).tobytes())
    # every byte value, scattered through an ordinary read
    r = np.frombuffer(ont_qual(100_000, ws), dtype=np.uint8).copy()
    pos = rng.choice(len(r), 256 * 3, replace=False)
    r[pos] = np.tile(np.arange(256, dtype=np.uint8), 3)
    reads.append(r.tobytes())
    # the read that stays ordinary up to one bad byte near its end
    r = np.frombuffer(ont_qual(60_000, ws + 1), dtype=np.uint8).copy()
    r[-3] = 200
    reads.append(r.tobytes())
    for L in (ws - 1, ws, ws + 1, 1000, 1023, 1024, 1025, 2047, 2048, 2049):
        if L >= 1:
            reads.append(ont_qual(L, L))
    return reads


@pytest.mark.parametrize("ws", [1, 7, 250, 1024, 5000])
@pytest.mark.parametrize("kernel", KERNELS)
def test_adversarial_data_through_the_path(ctx, ws, kernel, monkeypatch):
    monkeypatch.setenv("FLX_PHRED_LONG_MIN", "1000")
    set_kernel(monkeypatch, kernel)
    quals = adversarial_reads(ws) + [ont_qual(500, 3), b"", ont_qual(999, 4)]
    for order in ("desc", None):
        got, want, launches = score_both(ctx, quals, dict(window_size=ws, min_length=1000, min_window_q=20.0), order)
        assert_same(got, want, "ws=%d %s" % (ws, order))
        assert launches > 0


SKIP_WINDOWS = [7, 250, 700]  # 700 takes the dual-slot kernel by default
SKIP_ORDERS = (None, "random", "desc")


def skip_batch(ws, empties):
    """130 reads, two full waves and a tail of two, around a long threshold of 1000 bases.  In file order: a wave that mixes long, short
    and (with `empties`) empty reads, a wave of long reads only, a tail without a long read.  In descending order: a wave of long reads
    only, a wave with the other long reads, short ones and an empty one, a tail of two empty reads."""
    rng = np.random.default_rng(ws)
    lens = [0, 1, ws - 1, ws, ws + 1, 999, 1000, 1001, 0, 0]
    lens += [int(rng.integers(1000, 4000)) if i % 3 == 0 else int(rng.integers(2, 1000)) for i in range(54)]
    lens += [1000, 1001] + [int(L) for L in rng.integers(1000, 5000, 62)]
    lens += [500, 37]
    if not empties:
        lens = [L if L else 2 + i % 5 for i, L in enumerate(lens)]
    quals = [ont_qual(L, 7000 + i) if L else b"" for i, L in enumerate(lens)]
    for i in (5, 70):  # a byte >= 128 in a short and in a long read: the bank-private tables' redo list must not name a skipped read
        r = np.frombuffer(quals[i], dtype=np.uint8).copy()
        r[len(r) // 2] = 200
        quals[i] = r.tobytes()
    assert len(quals) == 130
    return quals


def wave_kinds(lengths, order, thr):
    """Per wave of 64 slots of the processing order: "long" (long reads only), "none", or "mixed" (long and other reads; "mixed+empty"
    if an empty read is among them)."""
    L = np.asarray(lengths)[order if order is not None else np.arange(len(lengths))]
    kinds = []
    for w in range(0, len(L), 64):
        lw = L[w:w + 64]
        n_long = int((lw >= thr).sum())
        kinds.append("long" if n_long == len(lw) else "none" if n_long == 0 else "mixed+empty" if (lw == 0).any() else "mixed")
    return kinds


def score_dev(ctx, packed, ws, order):
    """score_reads_dev over outputs pre-filled with sentinels (-1.0, -1.0, 7)."""
    import torch
    plane, offsets, lengths = packed
    n = len(lengths)
    d_plane = torch.from_numpy(plane).cuda()
    d_off = torch.from_numpy(offsets.view(np.int64)).cuda()
    d_len = torch.from_numpy(lengths).cuda()
    d_ord = torch.from_numpy(order.view(np.int32)).cuda() if order is not None else None
    mean = torch.full((n,), -1.0, dtype=torch.float64, device="cuda")
    win = torch.full((n,), -1.0, dtype=torch.float64, device="cuda")
    ok = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.score_reads_dev(d_plane.data_ptr(), len(plane), d_off.data_ptr(), d_len.data_ptr(), d_ord.data_ptr() if order is not None else None,
                        n, api.make_params(window_size=ws, min_length=200, min_window_q=30.0), mean.data_ptr(), win.data_ptr(), ok.data_ptr())
    torch.cuda.synchronize()
    return {"mean_q": mean.cpu().numpy(), "window_q": win.cpu().numpy(), "passed": ok.cpu().numpy(), "kernel": ctx.last_phred_kernel()}


def assert_no_sentinel(got, what):
    assert not (bits(got["mean_q"]) == bits([-1.0])[0]).any(), what + ": a mean was not written"
    assert not (bits(got["window_q"]) == bits([-1.0])[0]).any(), what + ": a window quality was not written"
    assert (got["passed"] <= 1).all(), what + ": a pass flag was not written"


@pytest.fixture(scope="module")
def skip_cases(ctx):
    """Per (window, empties): the packed batch, its three processing orders and the reference, FLX_PHRED_KERNEL=direct with the
    cooperative path off (one lane per read, byte by byte)."""
    cases = {}
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("FLX_PHRED_KERNEL", "direct")
        mp.setenv("FLX_PHRED_LONG_MIN", "0")
        for ws in SKIP_WINDOWS:
            for empties in (True, False):
                packed = api.pack_reads(skip_batch(ws, empties))
                lengths = packed[2]
                orders = {None: None, "random": np.random.default_rng(ws).permutation(len(lengths)).astype(np.uint32),
                          "desc": api.length_order(lengths)}
                want = score_dev(ctx, packed, ws, None)
                assert want["kernel"] == "flx_score_phred_direct"
                assert_no_sentinel(want, "reference ws=%d" % ws)
                cases[ws, empties] = (packed, orders, want)
    return cases


@pytest.mark.parametrize("ws", SKIP_WINDOWS)
@pytest.mark.parametrize("kernel", KERNELS)
def test_skip_inside_a_wave(ctx, skip_cases, kernel, ws, monkeypatch):
    """The batch kernel leaves the long reads of a wave alone and scores the others, empty ones included; the cooperative path writes
    the long ones: every field bit-identical to the direct kernel with the path off, no sentinel survives, an empty read has its NaN
    mean.  File order and descending order each hold a wave of long reads only, a wave without one and a wave that mixes long,
    short and empty reads; the random order mixes every full wave."""
    packed, orders, want = skip_cases[ws, True]
    lengths = packed[2]
    assert sorted(wave_kinds(lengths, orders[None], 1000)) == ["long", "mixed+empty", "none"]
    assert sorted(wave_kinds(lengths, orders["desc"], 1000)) == ["long", "mixed+empty", "none"]
    assert set(wave_kinds(lengths, orders["random"], 1000)[:2]) <= {"mixed", "mixed+empty"}
    monkeypatch.setenv("FLX_PHRED_LONG_MIN", "1000")
    set_kernel(monkeypatch, kernel)
    for name in SKIP_ORDERS:
        what = "%s ws=%d order=%s" % (kernel, ws, name)
        got = score_dev(ctx, packed, ws, orders[name])
        assert_no_sentinel(got, what)
        assert_same(got, want, what)
        assert np.isnan(got["mean_q"][lengths == 0]).all() and (lengths == 0).sum() == 3, what
        assert got["kernel"] != "flx_score_phred_long", what


@pytest.mark.parametrize("ws", SKIP_WINDOWS)
@pytest.mark.parametrize("kernel", KERNELS)
def test_every_read_skipped(ctx, skip_cases, kernel, ws, monkeypatch):
    """The same batch without its empty reads, every read long: the batch kernel is launched and writes nothing."""
    packed, orders, want = skip_cases[ws, False]
    assert (packed[2] >= 1).all()
    monkeypatch.setenv("FLX_PHRED_LONG_MIN", "1")
    set_kernel(monkeypatch, kernel)
    for name in SKIP_ORDERS:
        what = "%s ws=%d order=%s all long" % (kernel, ws, name)
        got = score_dev(ctx, packed, ws, orders[name])
        assert_no_sentinel(got, what)
        assert_same(got, want, what)
        assert got["kernel"] == "flx_score_phred_long", what


@pytest.fixture(scope="module")
def population():
    n = 100_000
    rng = np.random.default_rng(5)
    lens = np.minimum(rng.gamma(1.2, 900.0, n).astype(np.int64) + 1, 60_000)
    big = np.frombuffer(ont_qual(int(lens.sum()), 77), dtype=np.uint8)
    big = big.copy()
    big[rng.choice(len(big), 2000, replace=False)] = rng.integers(0, 256, 2000).astype(np.uint8)  # some negative qualities
    ends = np.cumsum(lens)
    quals = [big[e - L:e].tobytes() for e, L in zip(ends, lens)]
    quals[7] = b""
    return quals


@pytest.mark.parametrize("kernel", KERNELS)
def test_population_through_the_path(ctx, population, kernel, monkeypatch):
    """10^5 random reads, about 40 % of them >= 1000 bases and therefore through the cooperative path, the rest through the kernel
    FLX_PHRED_KERNEL selects, with no / a random / the descending processing order: bit-identical, and the path ran."""
    monkeypatch.setenv("FLX_PHRED_LONG_MIN", "1000")
    set_kernel(monkeypatch, kernel)
    pkw = dict(window_size=250, min_length=500, min_mean_q=80.0, min_window_q=55.0)
    want = None
    for order in (None, "random", "desc"):
        got, want, launches = score_both(ctx, population, pkw, order, want)
        assert_same(got, want, "%s order=%s" % (kernel, order))
        assert launches > 0, "the long-read path did not run"
    # the switch turns the path off: the same results from the default kernels alone
    monkeypatch.setenv("FLX_PHRED_LONG_MIN", "0")
    got, _, launches = score_both(ctx, population, pkw, "desc", want)
    assert_same(got, want, kernel + " path off")
    assert launches == 0


def test_ordinary_batch_does_not_take_the_path(ctx, population, monkeypatch):
    """No read reaches the threshold chosen from the data: nothing but the detection runs, the kernel choice is unchanged."""
    monkeypatch.delenv("FLX_PHRED_LONG_MIN", raising=False)
    got, want, launches = score_both(ctx, population[:20_000], dict(window_size=250))
    assert_same(got, want, "default threshold")
    assert launches == 0
    assert ctx.last_phred_kernel().startswith("flx_score_phred_regs")


def test_only_long_reads(ctx, long_reads, monkeypatch):
    """A batch of long reads only: nothing is left for the default kernels."""
    monkeypatch.delenv("FLX_PHRED_LONG_MIN", raising=False)
    got, want, launches = score_both(ctx, long_reads[:2], dict(window_size=250))
    assert_same(got, want, "only long")
    assert launches > 0 and ctx.last_phred_kernel() == "flx_score_phred_long"


@pytest.mark.parametrize("value", ["-1", "abc", "1.5", "", " 5", "+5"])
def test_switch_rejects_bad_values(ctx, value, monkeypatch):
    monkeypatch.setenv("FLX_PHRED_LONG_MIN", value)
    plane, offsets, lengths = api.pack_reads([ont_qual(100, 1)])
    with pytest.raises(api.FlxError, match="FLX_PHRED_LONG_MIN"):
        ctx.score_reads(plane, offsets, lengths, api.make_params())


@pytest.mark.parametrize("model", ["ont", "junk_stretches"])
def test_one_4mbp_read_is_fast(ctx, model, monkeypatch):
    """One 4 Mbp read, device-resident, window 250: the cooperative path takes at most a quarter of the one-lane fold's time.  For
    ONT-like qualities without junk stretches also under 5 ms.  Stretches whose 250-base windows hover at an average quality of
    0.5 (Phred ~3) change the window's binade every few bases and are folded serially by one wave: slower, but still
    far below the one-lane fold."""
    import torch
    if model == "ont":
        q = ont_qual(4_000_000, 1003, dips=0.0, centre=(9.0, 1.8))
    else:
        q = ont_qual(4_000_000, 1003)
    plane, offsets, lengths = api.pack_reads([q])
    d_plane = torch.from_numpy(plane).cuda()
    d_off = torch.from_numpy(offsets.view(np.int64)).cuda()
    d_len = torch.from_numpy(lengths).cuda()
    d_mean = torch.empty(1, dtype=torch.float64, device="cuda")
    d_win = torch.empty(1, dtype=torch.float64, device="cuda")
    d_pass = torch.empty(1, dtype=torch.uint8, device="cuda")
    params = api.make_params(window_size=250)

    def timed(reps):
        ts = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ctx.score_reads_dev(d_plane.data_ptr(), plane.nbytes, d_off.data_ptr(), d_len.data_ptr(), None, 1, params,
                                d_mean.data_ptr(), d_win.data_ptr(), d_pass.data_ptr())
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        return float(np.median(ts[2:])) * 1e3, (float(d_mean.item()), float(d_win.item()))

    monkeypatch.delenv("FLX_PHRED_LONG_MIN", raising=False)
    fast, r_fast = timed(9)
    monkeypatch.setenv("FLX_PHRED_LONG_MIN", "0")
    slow, r_slow = timed(5)
    print("4 Mbp read (%s): cooperative %.3f ms, one lane %.3f ms" % (model, fast, slow))
    assert bits(r_fast).tolist() == bits(r_slow).tolist()
    assert fast <= 0.25 * slow, (fast, slow)
    if model == "ont":
        assert fast < 5.0, (fast, slow)


def _fastq(tmp_path):
    rng = np.random.default_rng(11)
    recs = []
    lens = list(rng.integers(200, 12_000, 10_000)) + [1_000_000, 2_700_000, 4_000_000]
    order = rng.permutation(len(lens))
    for j, i in enumerate(order):
        L = int(lens[i])
        seq = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, L)].tobytes()
        recs.append(b"@r%d\n%s\n+\n%s\n" % (j, seq, ont_qual(L, 5000 + j, dips=0.01)))
    p = tmp_path / "reads.fastq"
    p.write_bytes(b"".join(recs))
    return str(p), sum(int(L) for L in lens)


def test_end_to_end_against_the_reference_binary(tmp_path):
    """10^4 ordinary reads and three of 1-4 Mbp through the command line — one process, and two forked ranks over the loopback
    communicator — with --target_bases and --keep_percent: stdout byte-identical to the reference binary's."""
    if not os.path.exists(_oracle.REF_FILTLONG):
        pytest.skip("reference binary not built")
    fq, total = _fastq(tmp_path)
    args = ["--target_bases", str(total // 3), "--keep_percent", "80", fq]
    env = dict(os.environ, LANG="C", LC_ALL="C")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "FLX_PHRED_LONG_MIN", "FLX_PHRED_KERNEL"):
        env.pop(k, None)
    ref = subprocess.run([_oracle.REF_FILTLONG] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
    assert ref.returncode == 0 and len(ref.stdout) > 0
    new = subprocess.run([BIN] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(env, FLX_API_TIMING="1"))
    assert new.returncode == 0, new.stderr[-500:]
    assert new.stdout == ref.stdout
    assert b"phred long reads" in new.stderr  # the cooperative path ran (FLX_API_TIMING stage line)
    shim_dir = os.path.join(ROOT, "tests", "shim")
    subprocess.check_call(["make", "-s", "-C", shim_dir])
    env2 = dict(env, FLX_RCCL_LIB=os.path.join(shim_dir, "libloopback_rccl.so"), FLX_DEVICE="0")
    new2 = subprocess.run([BIN, "--gpus", "2"] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env2)
    assert new2.returncode == 0, new2.stderr[-500:]
    assert new2.stdout == ref.stdout


def test_pipeline_with_small_chunks(ctx, monkeypatch):
    """flx_pipeline_*: chunks of a few hundred reads, the long reads among them (the slots grow for them): bit-identical."""
    monkeypatch.delenv("FLX_PHRED_LONG_MIN", raising=False)
    rng = np.random.default_rng(3)
    quals = [ont_qual(int(L), 900 + i) for i, L in enumerate(rng.integers(100, 8000, 3000))]
    for i, L in ((500, 1_200_000), (1700, 300_000), (2999, 2_000_000)):
        quals[i] = ont_qual(L, i)
    chunks = [quals[i:i + 400] for i in range(0, len(quals), 400)]
    pkw = dict(window_size=250, min_mean_q=70.0)
    got = ctx.score_stream(chunks, api.make_params(**pkw), chunk_bytes=1 << 20, chunk_reads=512, grow=True)
    plane, offsets, lengths = api.pack_reads(quals)
    want = _oracle.score_plane_mt(plane, offsets, lengths, _oracle.make_params(**pkw))
    assert_same(got, want, "pipeline")
