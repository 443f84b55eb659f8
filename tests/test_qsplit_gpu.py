"""--split_window_q on the GPU (csrc/qsplit.hip) against the model of tests/_qsplit_model.py: the child CSR, the ranges, first /
last and the wholly bad reads' flags for equality; the children's scores bit-equal to flx_score_batch over their quality substrings
and to the oracle's score_read.  Every test that expects splitting counts the reads that split (at least 2 children), the wholly bad
ones and the untouched ones: an input that never splits cannot pass."""
import numpy as np
import pytest

import _oracle
import _qsplit_model as model
from filtlong_amd import api

pytestmark = pytest.mark.gpu
STEP = 1024  # bases a wave takes per step of the detection kernel; a lane takes 16
PHRED = dict(good=(25, 40), junk=(0, 3))  # good bases that leave windows standing at Q = 99 (errors up to 0.003), junk that spoils them at Q = 50


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


def bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64)


def same_scores(got, want, what):
    for g, w, key in ((got[0], want[0], "mean_q"), (got[1], want[1], "window_q")):
        g, w = np.asarray(g, dtype=np.float64), np.asarray(w, dtype=np.float64)
        assert (np.isnan(g) == np.isnan(w)).all(), what + " " + key + ": NaN pattern differs"
        bad = np.nonzero((bits(g) != bits(w)) & ~np.isnan(w))[0]
        assert len(bad) == 0, "%s %s: %d of %d differ, first %d: got %s want %s" % (what, key, len(bad), len(w), bad[0], float(g[bad[0]]).hex(),
                                                                                  float(w[bad[0]]).hex())
    assert (np.asarray(got[2]) == np.asarray(want[2])).all(), what + " passed"


class Batch:
    """Reads packed once, and their scores without the flag per parameter set (computed once, never changed)."""

    def __init__(self, quals):
        self.quals = quals
        self.plane, self.offsets, self.lengths = api.pack_reads(quals)
        self.order = api.length_order(self.lengths)
        self.plain = {}

    def without_flag(self, ctx, pkw):
        key = tuple(sorted(pkw.items()))
        if key not in self.plain:
            self.plain[key] = ctx.score_reads(self.plane, self.offsets, self.lengths, api.make_params(**pkw), order=self.order)
        return self.plain[key]


def check_split(ctx, batch, w, q, pkw_extra=None, expect=("split", "wholly", "untouched"), child_capacity=None, got=None):
    """One call with the flag against the model, the library without the flag and the oracle.  Returns (result, census)."""
    pkw = dict(window_size=w, **(pkw_extra or {}))
    if got is None:
        got = ctx.score_reads(batch.plane, batch.offsets, batch.lengths, api.make_params(**pkw), order=batch.order, split_window_q=q,
                              child_capacity=child_capacity)
    what = "W=%d Q=%g" % (w, q)
    off, rng, first, last, wholly = model.split_batch(batch.quals, w, q)
    assert (got["child_offsets"] == off).all(), what + " child_offsets"
    assert got["child_ranges"].shape == rng.shape and (got["child_ranges"] == rng).all(), what + " child_ranges"
    assert (got["first"] == first).all() and (got["last"] == last).all(), what + " first/last"
    # the parents: today's scores; a wholly bad read fails
    plain = batch.without_flag(ctx, pkw)
    want_pass = np.where(wholly, 0, plain["passed"]).astype(np.uint8)
    same_scores((got["mean_q"], got["window_q"], got["passed"]), (plain["mean_q"], plain["window_q"], want_pass), what + " parents")
    # the children: each a read of its own
    parent = np.repeat(np.arange(len(batch.quals)), np.diff(off.astype(np.int64)))
    subs = [batch.quals[p][s:e] for p, (s, e) in zip(parent, rng)]
    if subs:
        cplane, coff, clen = api.pack_reads(subs)
        assert (clen == rng[:, 1] - rng[:, 0]).all() and (clen > 0).all()
        lib = ctx.score_reads(cplane, coff, clen, api.make_params(**pkw), order=api.length_order(clen))
        orc = _oracle.score_plane_mt(cplane, coff, clen, _oracle.make_params(**pkw))
        kids = (got["child_mean_q"], got["child_window_q"], got["child_passed"])
        same_scores(kids, (lib["mean_q"], lib["window_q"], lib["passed"]), what + " children vs flx_score_batch")
        same_scores(kids, (orc["mean_q"], orc["window_q"], orc["passed"]), what + " children vs the oracle")
    census = dict(zip(("split", "wholly", "untouched"), model.census(off, wholly)))
    for k in expect:
        assert census[k] > 0, "%s: no %s read in the input (%r)" % (what, k, census)
    return got, census


@pytest.fixture(scope="module")
def random_batch():
    """About 2000 reads of 0..3000 bases with random junk stretches (Phred 0-3 in Phred 25-40), some of them all junk, some with a
    stretch long enough to spoil a window of 1000 bases in their middle."""
    rng = np.random.default_rng(4242)
    quals = []
    for i in range(2000):
        length = int(rng.integers(0, 3001))
        k = int(rng.integers(0, 4))
        st = [(int(a), int(a) + int(rng.integers(1, 500))) for a in rng.integers(0, max(length, 1), size=k)]
        if i % 40 == 0:
            st = [(0, length)]
        quals.append(model.junk_read(rng, length, st, **PHRED))
    for i in range(24):
        a = 1050 + 10 * i
        quals.append(model.junk_read(rng, 3000, [(a, a + 800)], **PHRED))
    quals += [b"", b"!" * 700, b"~" * 700]
    return Batch(quals)


@pytest.mark.parametrize("q", [50, 85, 90, 99])
@pytest.mark.parametrize("w", [1, 2, 7, 31, 250, 251, 1000])
def test_library_against_the_model(ctx, random_batch, w, q):
    _, census = check_split(ctx, random_batch, w, q)
    if w == 1000:
        assert ctx.last_phred_kernel() == "flx_score_phred_dual"  # (the children's call is the context's last)


@pytest.mark.parametrize("pkw", [dict(min_length=200), dict(min_window_q=80.0), dict(min_length=100, min_window_q=90.0, min_mean_q=93.0, max_length=1500)])
def test_child_passed_under_the_hard_cutoffs(ctx, random_batch, pkw):
    got, _ = check_split(ctx, random_batch, 250, 85, pkw)
    assert 0 < int(got["child_passed"].sum()) < len(got["child_passed"])


def edge_reads():
    """Read lengths and junk positions at the wave step +-1 and at the 16-byte lane boundaries +-1."""
    rng = np.random.default_rng(9)
    quals = []
    for length in (15, 16, 17, 31, 32, 33, STEP - 1, STEP, STEP + 1, 2 * STEP - 1, 2 * STEP, 2 * STEP + 1, 3 * STEP + 7):
        quals.append(model.junk_read(rng, length, [], **PHRED))
        for at in (0, 15, 16, 17, STEP - 17, STEP - 16, STEP - 1, STEP, STEP + 1, STEP + 15, STEP + 16, 2 * STEP - 1, 2 * STEP, length - 1):
            for n in (1, 2, 16, 17):
                if 0 <= at < length:
                    quals.append(model.junk_read(rng, length, [(at, at + n)], **PHRED))
    return quals


@pytest.fixture(scope="module")
def edge_batch():
    return Batch(edge_reads())


@pytest.mark.parametrize("w,q", [(1, 85), (2, 85), (7, 85), (16, 90), (17, 90), (250, 99), (STEP - 1, 99), (STEP, 99), (STEP + 1, 99)])
def test_step_and_lane_boundaries(ctx, edge_batch, w, q):
    check_split(ctx, edge_batch, w, q, expect=("split", "untouched"))


def test_one_long_read_with_stretches_across_steps(ctx, monkeypatch):
    """300 000 bases, junk stretches straddling step boundaries; with FLX_PHRED_LONG_MIN=4096 its children take the cooperative path."""
    monkeypatch.setenv("FLX_PHRED_LONG_MIN", "4096")
    rng = np.random.default_rng(31)
    st = [(k * STEP - 40, k * STEP + 60) for k in (3, 50, 51, 120, 200)] + [(100 * STEP - 1, 100 * STEP + 1), (150_000, 151_500), (299_900, 300_000)]
    batch = Batch([model.junk_read(rng, 300_000, st, **PHRED), model.junk_read(rng, 5000, [(2000, 2300)], **PHRED), b"~" * 100])
    ctx.timing_enable(True)
    ctx.timing_reset()
    got, _ = check_split(ctx, batch, 250, 85, expect=("split", "untouched"))
    long_launches = ctx.timing_get("flx_score_phred_long")[1]
    detect_launches = ctx.timing_get("flx_qsplit_detect")[1]
    ctx.timing_enable(False)
    assert (got["child_ranges"][:, 1] - got["child_ranges"][:, 0]).max() > 4096 and long_launches > 0
    assert detect_launches == 2  # the count pass and the emit pass


def test_tens_of_thousands_of_children_from_one_read(ctx):
    """100 000 bases, W = 1, alternating qualities: 50 000 children of one base from one read, through the capacity retry; an all-'!' read
    whose window sums need 64 bits; children of exactly 1023 and 1024 bases (the 128-byte start rule of the child plane)."""
    quals = [b"~!" * 50_000, b"!" * 5000, b"~" * 1023 + b"!" + b"~" * 1024, b"~" * 1024 + b"!" + b"~" * 1023 + b"!" + b"~" * 5, b"~" * 300]
    batch = Batch(quals)
    got, census = check_split(ctx, batch, 1, 85, child_capacity=16)
    per = np.diff(got["child_offsets"].astype(np.int64))
    assert list(per) == [50_000, 0, 2, 3, 0] and census["wholly"] == 1
    lens = got["child_ranges"][:, 1] - got["child_ranges"][:, 0]
    assert list(lens[50_000:]) == [1023, 1024, 1024, 1023, 5]
    # the same reads with a window of 250: the sums of the all-'!' read are 250 * (2^32 - 1)
    check_split(ctx, batch, 250, 50, expect=("wholly",))
    # the error the retry answers: the capacity needed comes back in n_children
    import ctypes as C
    s = api.Scores()
    n = len(quals)
    arrays = [np.zeros(n, np.float64), np.zeros(n, np.float64), np.zeros(n, np.uint8), np.zeros(n + 1, np.uint64), np.zeros(32, np.int32),
              np.zeros(16, np.float64), np.zeros(16, np.float64), np.zeros(16, np.uint8)]
    s.mean_q, s.window_q, s.passed, s.child_offsets, s.child_ranges, s.child_mean_q, s.child_window_q, s.child_passed = [a.ctypes.data for a in arrays]
    s.child_capacity = 16
    rc = ctx.L.flx_score_batch_qsplit(ctx.h, batch.plane.ctypes.data, batch.plane.nbytes, batch.offsets.ctypes.data, batch.lengths.ctypes.data, None, n,
                                      C.byref(api.make_params(window_size=1)), 85.0, C.byref(s))
    assert rc == 5 and s.n_children == 50_005


def test_pipeline_equals_one_call(ctx, random_batch):
    """The same reads through flx_pipeline_* in chunks of a few reads: the children are concatenated across the slots and the child
    capacity (1024 at first for chunks of 64 reads) grows: the W = 1 chunk of the alternating read alone has 50 000."""
    quals = random_batch.quals[:400] + [b"~!" * 50_000] + random_batch.quals[400:700]
    batch = Batch(quals)
    for w, q in ((1, 85), (250, 85)):
        one, _ = check_split(ctx, batch, w, q)
        chunks = [quals[i:i + 37] for i in range(0, len(quals), 37)]
        got = ctx.score_stream(chunks, api.make_params(window_size=w), chunk_bytes=1 << 18, chunk_reads=64, split_window_q=q)
        for key in ("child_offsets", "child_ranges", "first", "last", "passed", "child_passed"):
            assert got[key].shape == one[key].shape and (got[key] == one[key]).all(), (w, key)
        same_scores((got["mean_q"], got["window_q"], got["passed"]), (one["mean_q"], one["window_q"], one["passed"]), "pipeline parents")
        same_scores((got["child_mean_q"], got["child_window_q"], got["child_passed"]),
                    (one["child_mean_q"], one["child_window_q"], one["child_passed"]), "pipeline children")


def test_setter_is_refused_where_it_does_not_apply(ctx):
    import ctypes as C
    L = ctx.L
    pipe = C.c_void_p()
    ctx._check(L.flx_pipeline_create(ctx.h, None, C.byref(api.make_params()), 1 << 16, 16, C.byref(pipe)))
    try:
        assert L.flx_pipeline_set_qsplit(pipe, 0.0) == 1 and L.flx_pipeline_set_qsplit(pipe, 100.0) == 1
        assert L.flx_pipeline_set_qsplit(pipe, 85.0) == 0
        buf = C.c_void_p()
        ctx._check(L.flx_pipeline_next_buffer(pipe, C.byref(buf), None, None))
        ctx._check(L.flx_pipeline_submit(pipe, 0, None, None, 0))
        assert L.flx_pipeline_set_qsplit(pipe, 85.0) == 4  # FLX_ERR_STATE: after a submit
    finally:
        L.flx_pipeline_destroy(pipe)
    with pytest.raises(api.FlxError):
        ctx.score_reads(*api.pack_reads([b"~" * 10]), api.make_params(), split_window_q=100.0)


def test_nothing_moves_without_the_flag(ctx, random_batch):
    """Without the flag a Phred batch launches what it launched before: the Phred kernels and nothing of qsplit.hip; first / last stay -1
    and there are no children."""
    ctx.timing_enable(True)
    ctx.timing_reset()
    got = ctx.score_reads(random_batch.plane, random_batch.offsets, random_batch.lengths, api.make_params(), order=random_batch.order)
    kernel = ctx.last_phred_kernel()
    everything, phred, qsplit = ctx.timing_get("")[1], ctx.timing_get("flx_score_phred")[1], ctx.timing_get("flx_qsplit")[1]
    ctx.timing_enable(False)
    assert kernel in ("flx_score_phred_regs", "flx_score_phred_regs_private")
    assert qsplit == 0 and phred >= 1 and everything == phred
    assert (got["first"] == -1).all() and (got["last"] == -1).all() and (got["child_offsets"] == 0).all() and len(got["child_mean_q"]) == 0
    want = _oracle.score_plane_mt(random_batch.plane, random_batch.offsets, random_batch.lengths, _oracle.make_params())
    same_scores((got["mean_q"], got["window_q"], got["passed"]), (want["mean_q"], want["window_q"], want["passed"]), "without the flag")
