"""The k-mer fold kernels (k_kmer_fold<MODE, RING, GRID>, filtlong_amd/csrc/score_kmer.hip) in every form launch_fold can pick, against the
oracle — bit exact — with an assertion of WHICH form ran.

launch_fold picks the form from the window size alone: ring words per lane R = 32, doubled while R < base + ceil(ws / 32), base = 18 for
the parent modes (0 .. 5) and 24 for the one-lane-per-child mode 6; R <= 512 runs the LDS ring (four waves per workgroup up to R = 64, one
wave above), R > 512 streams both window edges from global memory.  So parents change class after ws = 448, 1472, 3520, 7616, 15808 and
children after 256, 1280, 3328, 7424, 15616 (the literal tables below: if the thresholds in the library move, these tests fail instead of
quietly testing something else).  Every fold launch has a timing bracket named after its form (flx_score_kmer_fold.m<mode>.<ring<R> |
global>.<fp | grid>, and flx_score_kmer_fold.inline for k_children_from_inline): the tests read them back with Context.timing_get.

Window sizes: every remainder ws % 32 twice (ws = 1 .. 66, 225 .. 257: the alignbit shift of the trailing word, the place of the first
full window inside a word, the `j0 + 32 <= ws - 1` head shortcut), both sides of every class edge, windows inside the classes R = 256 and
R = 512, and windows beyond the ring (20011, 32768: the global streams for their real reason).

The read set of a window size (build_reads): parents at ws - 1, ws, ws + 1, ws + 31, ws + 32, ws + 33, 2 ws -+ 1, 3 ws + 5 and random lengths;
every parent is made of clean stretches of the assembly (1.2 .. 3 ws, + 64 bases so that a child of a small window is longer than the window
too) separated by junk blocks at least --split long; substitutions on a third of the reads, an all-junk read, a read shorter than 16, a read
with a child shorter than the window, a read with exactly 8 children (what fits inline) and — where asked — one with 11 (MODE 5 must run).
A 16-mer of random junk occurs in the 400 kbase assembly with probability 2e-4, so junk is not always uncovered: the oracle says what is
right, and what a test needs from its inputs (long parents and children, short ones, windows that differ from the mean, the child counts
that decide about MODE 5) is asserted from the oracle's output, before the device runs.
"""
import bisect
from types import SimpleNamespace

import numpy as np
import pytest

import _cases
import _oracle
from filtlong_amd import api

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
PREFIX = "flx_score_kmer_fold"
# ring words per lane: the last window size of every class (32, 64, 128, 256, 512 words; beyond the last one: global streams)
PARENT_EDGES = (448, 1472, 3520, 7616, 15808)
CHILD_EDGES = (256, 1280, 3328, 7424, 15616)
PATHS = ("ring32", "ring64", "ring128", "ring256", "ring512", "global")


def fold_path(ws, mode):
    return PATHS[bisect.bisect_left(CHILD_EDGES if mode == 6 else PARENT_EDGES, ws)]


def ring_rule(ws, mode):
    """launch_fold's rule as the library states it (the literal edges above must say the same)."""
    R = 32
    while R < (24 if mode == 6 else 18) + (ws + 31) // 32:
        R *= 2
    return "ring%d" % R if R <= 512 else "global"


def default_split(ws):
    return max(32, ws // 8)


# ------------------------------------------------------------------------------------------------------------------ inputs
def _junk_len(rng, split):
    """A junk block's length: the clean stretch in front of it goes on into the junk while its bases agree with the assembly by chance
    (one in four does), so a block of exactly --split bases may leave a shorter zero run — 8 bases more."""
    return int(rng.randint(split + 8, split + split // 2 + 10))


def _junk(rng, n, quiet=False):
    if quiet:  # a tandem repeat of a random 5-mer: five 16-mers and their reverse complements, absent from the assembly (asserted through the child counts)
        return np.resize(ACGT[rng.randint(0, 4, 5)], n)
    return ACGT[rng.randint(0, 4, n)]


def _clean(ref, rng, n):
    s0 = int(rng.randint(0, len(ref) - n))
    return ref[s0:s0 + n]


def _parent(ref, rng, L, ws, split):
    seq = np.empty(L, dtype=np.uint8)
    pos, junk_now, n_junk = 0, rng.rand() < 0.5, 0
    while pos < L:
        if junk_now:
            n = min(L - pos, _junk_len(rng, split))
            seq[pos:pos + n] = _junk(rng, n)
            n_junk += 1
        else:
            n = min(L - pos, int(rng.uniform(1.2, 3.0) * ws) + 64)
            seq[pos:pos + n] = _clean(ref, rng, n)
        pos += n
        junk_now = not junk_now
    if n_junk == 0 and L >= 48:  # a read that one clean stretch fills: its window would be its mean
        n = min(split, L // 3)
        at = int(rng.randint(0, L - n + 1))
        seq[at:at + n] = _junk(rng, n)
    return seq


def _islands(ref, rng, lens, split, lead=True):
    """Clean stretches of the given lengths between quiet junk blocks of split .. 1.5 split bases: under --trim --split one child each."""
    parts = [_junk(rng, _junk_len(rng, split), quiet=True)] if lead else []
    for n in lens:
        parts.append(_clean(ref, rng, n))
        parts.append(_junk(rng, _junk_len(rng, split), quiet=True))
    return np.concatenate(parts)


def build_reads(ref, ws, n_reads, seed, lo=None, hi=None, overflow=False):
    """The read set of a window size (module docstring), in file order: the read shorter than 16 sits among the long ones of the first wave."""
    rng = np.random.RandomState(seed)
    split = default_split(ws)
    lengths = [max(1, ws - 1), ws, ws + 1, ws + 31, ws + 32, ws + 33, max(1, 2 * ws - 1), 2 * ws + 1, 3 * ws + 5]
    special = 6 if overflow else 5
    n_random = max(8, n_reads - len(lengths) - special)
    lo = ws + 64 if lo is None else lo
    hi = max(lo + 1, int(3.2 * ws)) if hi is None else hi
    lengths += [int(x) for x in rng.randint(lo, hi + 1, n_random)]
    rng.shuffle(lengths)
    reads = [_parent(ref, rng, L, ws, split) for L in lengths]
    for k in range(0, len(reads), 3):  # 2 % substitutions on a third of them
        sub = rng.rand(len(reads[k])) < 0.02
        reads[k][sub] = ACGT[rng.randint(0, 4, int(sub.sum()))]
    short = max(17, min(ws // 2, 200))  # a child shorter than the window (when the window is longer than a 16-mer's coverage)
    extra = [_clean(ref, rng, 9),                                                                  # shorter than 16: no 16-mer at all
             _junk(rng, ws + 100),                                                                 # all junk
             _islands(ref, rng, [short, int(1.3 * ws) + 64], split),
             _islands(ref, rng, [int(x) for x in rng.randint(40, 90, 8)], split),                  # exactly 8 children
             _islands(ref, rng, [int(1.2 * ws) + 64, 40, 70], split, lead=False)]
    if overflow:
        extra.append(_islands(ref, rng, [int(x) for x in rng.randint(40, 90, 11)], split))     # more than fit inline
    for k, r in enumerate(extra):  # spread over the batch, the tiny read at index 5
        reads.insert(min(len(reads), 5 + 7 * k), r)
    return [r.tobytes() for r in reads]


def prepare(env, ws, n_reads, param_sets, seed=None, overflow=None, lo=None, hi=None):
    """Reads, the oracle's result per parameter set, and the conditions that keep a comparison from passing on nothing."""
    reads = build_reads(env.ref, ws, n_reads, 1000 + ws if seed is None else seed, lo=lo, hi=hi, overflow=overflow)
    plane, offsets, lengths = api.pack_reads(reads)
    case = SimpleNamespace(ws=ws, plane=plane, offsets=offsets, lengths=lengths, overflow=overflow, want={}, pkws={})
    for tag, pkw in param_sets.items():
        want = _oracle.score_plane_mt(plane, offsets, lengths, _oracle.make_params(**pkw), kmerset=env.oset, child_cap=int(lengths.sum()) // 16 + 64)
        case.want[tag], case.pkws[tag] = want, pkw
        L = lengths.astype(np.int64)
        steady = L > ws
        assert int((L >= ws + 64).sum()) >= 8, (ws, tag, "long parents")
        if ws >= 2:
            assert (L < ws).any(), (ws, tag, "a parent shorter than the window")
        differs = want["window_q"][steady] != want["mean_q"][steady]
        assert 2 * int(differs.sum()) >= int(steady.sum()) > 0, (ws, tag, "windows that differ from the mean")
        if pkw.get("trim") or pkw.get("split") is not None:
            assert want["n_children"] > 0, (ws, tag)
            per_read = np.diff(want["child_offsets"].astype(np.int64))
            if pkw["split"] >= 32:  # the read sets are built for the word-level child passes; --split 20 runs on the same reads
                clen = (want["child_ranges"][:, 1] - want["child_ranges"][:, 0]).astype(np.int64)
                assert int((clen >= ws + 64).sum()) >= 8, (ws, tag, "long children")
                if ws >= 32:
                    assert (clen < ws).any(), (ws, tag, "a child shorter than the window")
                assert (per_read == 8).any(), (ws, tag, "a read with exactly 8 children")
                if overflow is not None:  # MODE 5 must run / must not run
                    assert (per_read.max() >= 9) == overflow, (ws, tag, "children per read", int(per_read.max()))
    return case


def expected_launches(ws, pkw, n_children, most_children, grid_ran, fold_env=None, streams_global=False):
    """Timing names and counts of the fold launches of one scoring call (flx_score_kmer_dev)."""
    def name(mode):
        path = "global" if streams_global else fold_path(ws, mode)
        arith = "grid" if grid_ran and mode in (0, 3, 6) and path != "global" else "fp"
        return "%s.m%d.%s.%s" % (PREFIX, mode, path, arith)

    split = pkw.get("split")
    if not (pkw.get("trim") or split is not None):
        return {name(0): 1}
    bit_level = (split is not None and split < 32) or fold_env == "bits"
    exp = {name(1 if bit_level else 3): 1}
    if n_children > 0:
        if bit_level:
            exp[name(2)] = 1
        elif fold_env == "words":
            exp[name(4)] = 1
        else:
            exp[PREFIX + ".inline"] = 1
            if most_children > 8:
                exp[name(5)] = 1
            exp[name(6)] = 1
    return exp


def expected_grid(ws, pkw, fold_env=None, grid_env=None, streams_global=False):
    """What flx_last_kmer_fold_grid must say where it is known; None: the window's grid table decides (build_grid_table)."""
    split = pkw.get("split")
    bit_level = (split is not None and split < 32) or fold_env == "bits"
    if bit_level or grid_env == "0" or streams_global or fold_path(ws, 0) == "global" or ws < 8 or ws == 1000:
        return False
    if ws & (ws - 1) == 0:
        return True  # a power of two: the step is exact on every binade
    return None


def run_device(env, case, tag, order, monkeypatch, fold_env=None, grid_env=None, streams_global=False):
    ctx, ws, pkw, want = env.ctx, case.ws, case.pkws[tag], case.want[tag]
    for var, val in (("FLX_KMER_FOLD", fold_env), ("FLX_KMER_FOLD_GRID", grid_env), ("FLX_KMER_FOLD_STREAMS", "global" if streams_global else None)):
        if val is None:
            monkeypatch.delenv(var, raising=False)
        else:
            monkeypatch.setenv(var, val)
    what = (ws, tag, "file order" if order is None else "length order", fold_env, grid_env, streams_global)
    ctx.timing_reset()
    dev = ctx.score_reads(case.plane, case.offsets, case.lengths, api.make_params(**pkw), kmers=env.ks, order=order,
                          child_capacity=want["n_children"] + 16)  # (room for all: a second call would double the brackets)
    _cases.same(dev, want, what)
    grid_ran = ctx.last_kmer_fold_grid()
    known = expected_grid(ws, pkw, fold_env, grid_env, streams_global)
    if known is not None:
        assert grid_ran == known, what
    per_read = np.diff(want["child_offsets"].astype(np.int64))
    exp = expected_launches(ws, pkw, want["n_children"], int(per_read.max()), grid_ran, fold_env, streams_global)
    for name, count in exp.items():
        assert ctx.timing_get(name)[1] == count, (what, name, exp)
    assert ctx.timing_get(PREFIX)[1] == sum(exp.values()), (what, exp)  # nothing else under the prefix: no bracket nests
    for var in ("FLX_KMER_FOLD", "FLX_KMER_FOLD_GRID", "FLX_KMER_FOLD_STREAMS"):
        monkeypatch.delenv(var, raising=False)
    return exp


def check_window(env, ws, n_reads, monkeypatch, lo=None, hi=None, overflow=None):
    """One window size: window alone and --trim --split, in length order and in file order."""
    for mode in (0, 6):
        assert fold_path(ws, mode) == ring_rule(ws, mode), (ws, mode)
    case = prepare(env, ws, n_reads, {"window": dict(window_size=ws), "trim+split": dict(window_size=ws, trim=True, split=default_split(ws))},
                   lo=lo, hi=hi, overflow=overflow)
    order = api.length_order(case.lengths)
    ran = {}
    for tag in case.pkws:
        for o in (order, None):  # file order: the short reads share a wave with long ones, the word-level shortcuts (Lmin) switch off
            ran.update(run_device(env, case, tag, o, monkeypatch))
    # the forms this window size is here for
    assert any(k.startswith("%s.m0.%s." % (PREFIX, fold_path(ws, 0))) for k in ran), (ws, ran)
    assert any(k.startswith("%s.m3.%s." % (PREFIX, fold_path(ws, 3))) for k in ran), (ws, ran)
    assert any(k.startswith("%s.m6.%s." % (PREFIX, fold_path(ws, 6))) for k in ran), (ws, ran)
    return ran


# ------------------------------------------------------------------------------------------------------------------ fixtures
@pytest.fixture(scope="module")
def env():
    from filtlong_amd import synth as S
    ctx = api.Context(0)
    ref = S.bases_read(S.STREAM_REF, 0, 0, 400_000)
    oset = _oracle.KmerSet()
    oset.add_assembly([ref.tobytes()])
    ks = api.Kmers(ctx)
    ks.add_assembly_fasta([ref.tobytes()])
    ks.finalize()
    assert len(ks) == len(oset)
    ctx.timing_enable(True)
    yield SimpleNamespace(ctx=ctx, ref=ref, oset=oset, ks=ks)
    ks.close()
    ctx.close()


def batch_size(ws):
    """Fewer than 64 reads, exactly one wave, two waves and a tail of two (where the window size allows): a window size and the
    one 32 further on — the same remainder — get different kinds."""
    if ws > 3600:
        return 66 if ws in (5000, 12000, 20011) else 24  # (one wave per workgroup from R = 128 on: two workgroups, the second with two reads)
    return (24, 64, 130)[ws % 3] if ws <= 1500 else (24, 64)[ws % 2]


# ------------------------------------------------------------------------------------------------------------------ tests
REMAINDER_GROUPS = [range(1, 17), range(17, 33), range(33, 50), range(50, 67), range(225, 241), range(241, 258)]


@pytest.mark.parametrize("group", REMAINDER_GROUPS, ids=lambda g: "ws%d-%d" % (g[0], g[-1]))
def test_every_window_remainder(env, monkeypatch, group):
    """ws = 1 .. 66 and 225 .. 257: all 32 values of ws % 32 twice or more, across the children's first class edge (256 | 257), on reads
    of 600 .. 3000 bases (and the parents at the window's own size)."""
    for ws in group:
        ran = check_window(env, ws, batch_size(ws), monkeypatch, lo=600, hi=3000)
        assert any(".m0.ring32." in k for k in ran) and any(".m3.ring32." in k for k in ran), (ws, ran)
        assert any((".m6.ring32." if ws <= 256 else ".m6.ring64.") in k for k in ran), (ws, ran)


# window size -> (parents' form, children's form) on both sides of every class edge
EDGE_FORMS = {448: ("ring32", "ring64"), 449: ("ring64", "ring64"), 1280: ("ring64", "ring64"), 1281: ("ring64", "ring128"),
              1472: ("ring64", "ring128"), 1473: ("ring128", "ring128"), 3328: ("ring128", "ring128"), 3329: ("ring128", "ring256"),
              3520: ("ring128", "ring256"), 3521: ("ring256", "ring256"), 7424: ("ring256", "ring256"), 7425: ("ring256", "ring512"),
              7616: ("ring256", "ring512"), 7617: ("ring512", "ring512"), 15616: ("ring512", "ring512"), 15617: ("ring512", "global"),
              15808: ("ring512", "global"), 15809: ("global", "global")}


@pytest.mark.parametrize("ws", sorted(EDGE_FORMS))
def test_both_sides_of_every_class_edge(env, monkeypatch, ws):
    """The last window size of a class and the first of the next, for the parents' edges and for the children's; between a children's edge
    and the parents' next one the two run different classes in one call (15616 < ws <= 15808: children from global memory, parents
    through the ring)."""
    parents, children = EDGE_FORMS[ws]
    assert (fold_path(ws, 0), fold_path(ws, 3), fold_path(ws, 6)) == (parents, parents, children)
    ran = check_window(env, ws, batch_size(ws), monkeypatch, overflow=False)
    for mode, path in ((0, parents), (3, parents), (6, children)):
        assert [k for k in ran if ".m%d." % mode in k and ".%s." % path not in k] == [], (ws, ran)
    assert not any(".m5." in k for k in ran), (ws, ran)  # no read has more children than fit inline: the ranges pass must not run


@pytest.mark.parametrize("ws", [4096, 5000, 8192, 12000])
def test_inside_the_long_rings(env, monkeypatch, ws):
    """R = 256 and R = 512 in steady state (one wave per workgroup, 64 and 128 KiB of LDS).  4096 and 8192: a power of two makes the
    step exact, so the integer-grid kernel must run at that size of ring."""
    ran = check_window(env, ws, batch_size(ws), monkeypatch, overflow=False)
    ring = "ring256" if ws <= 7424 else "ring512"
    arith = "grid" if ws in (4096, 8192) else None
    for mode in (0, 3, 6):
        names = [k for k in ran if k.startswith("%s.m%d.%s." % (PREFIX, mode, ring))]
        assert names and (arith is None or all(k.endswith("." + arith) for k in names)), (ws, mode, ran)


@pytest.mark.parametrize("ws", [20011, 32768])
def test_windows_beyond_the_ring(env, monkeypatch, ws):
    """Windows too long for 512 ring words: parents and children stream both window edges from global memory, without any switch."""
    ran = check_window(env, ws, batch_size(ws), monkeypatch, overflow=False)
    assert sorted(k for k in ran if ".m" in k) == ["%s.m%d.global.fp" % (PREFIX, m) for m in (0, 3, 6)], (ws, ran)


@pytest.mark.parametrize("ws", [250, 1000, 2047, 5000, 12000, 20011])
def test_forced_forms_and_child_overflow_per_class(env, monkeypatch, ws):
    """Once per class (R = 32, 64, 128, 256, 512, global): the ranges pass for a batch in which a read has more children than fit inline
    (MODE 5 runs; without such a read it must not), the bit-level passes for --split 20 (MODE 1, 2), and the forced forms —
    FLX_KMER_FOLD=words (MODE 4), =bits, FLX_KMER_FOLD_GRID=0, FLX_KMER_FOLD_STREAMS=global — all against the oracle, with their names."""
    sets = {"trim+split": dict(window_size=ws, trim=True, split=default_split(ws)), "split20": dict(window_size=ws, split=20),
            "window": dict(window_size=ws)}
    case = prepare(env, ws, 24, sets, seed=5000 + ws, overflow=True)
    order = api.length_order(case.lengths)
    for o in (order, None):
        exp = run_device(env, case, "trim+split", o, monkeypatch)
        assert exp["%s.m5.%s.fp" % (PREFIX, fold_path(ws, 5))] == 1 and exp[PREFIX + ".inline"] == 1, (ws, exp)
        exp = run_device(env, case, "split20", o, monkeypatch)
        assert sorted(exp) == ["%s.m%d.%s.fp" % (PREFIX, m, fold_path(ws, m)) for m in (1, 2)], (ws, exp)
    exp = run_device(env, case, "trim+split", order, monkeypatch, fold_env="words")
    assert "%s.m4.%s.fp" % (PREFIX, fold_path(ws, 4)) in exp and len(exp) == 2, (ws, exp)
    exp = run_device(env, case, "trim+split", order, monkeypatch, fold_env="bits")
    assert sorted(exp) == ["%s.m%d.%s.fp" % (PREFIX, m, fold_path(ws, m)) for m in (1, 2)], (ws, exp)
    for tag in ("window", "trim+split"):
        exp = run_device(env, case, tag, order, monkeypatch, grid_env="0")
        assert all(k.endswith(".fp") or k.endswith(".inline") for k in exp), (ws, exp)
    if fold_path(ws, 0) != "global":  # the round-2 data path where the ring would have fitted
        for tag in ("window", "trim+split"):
            exp = run_device(env, case, tag, order, monkeypatch, streams_global=True)
            assert all(".global.fp" in k or k.endswith(".inline") for k in exp), (ws, exp)
