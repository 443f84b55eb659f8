"""The global stage over the children of --split_window_q: flx_reads2_gather and flx_rank_and_cut* (both device forms of the cut, and
the sharded select) over a reads2 made of Phred children, against the oracle's reads2 gather and rank_and_cut over the children
of tests/_qsplit_model.py scored by the oracle's score_read.  The input holds exact duplicates of reads that split, so children tie
bit for bit and a target can fall inside such a group; wholly bad reads stay in reads2 as failing entries that still count in the
quality statistics; total_bases is the input's bases, not reads2's.  Everything is compared for equality."""
import os
import re

import numpy as np
import pytest

import _oracle
import _pipeline
import _qsplit_model as model
from filtlong_amd import api
from test_gpu_sharded import check_out, even

pytestmark = pytest.mark.gpu
W, Q = 250, 85
PKW = dict(window_size=W)
PHRED = dict(good=(25, 40), junk=(0, 3))
CHILD_NAME = re.compile(r"_\d+-\d+$")  # name_start-end


def made_reads():
    """400 reads of 300..4000 bases (a quarter untouched, half with one junk stretch, a quarter with two, every fifteenth wholly junk,
    one shorter than the window) and 40 exact duplicates of reads that split."""
    rng = np.random.default_rng(808)
    reads = []
    for i in range(400):
        length = int(rng.integers(300, 4000)) if i != 7 else 120
        k = (0, 1, 2, 1)[i % 4]
        st = [(int(a), int(a) + int(rng.integers(40, 400))) for a in rng.integers(0, length, size=k)]
        if i % 15 == 4:
            st = [(0, length)]
        seq = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=length).tobytes()
        reads.append(("read_%d" % i, seq, model.junk_read(rng, length, st, **PHRED)))
    off, _, _, _, _ = model.split_batch([r[2] for r in reads], W, Q)
    splitting = np.flatnonzero(np.diff(off.astype(np.int64)) >= 2)
    assert len(splitting) >= 40
    for k, i in enumerate(rng.choice(splitting, size=40, replace=False)):
        reads.append(("dup_%d_of_%d" % (k, i), reads[i][1], reads[i][2]))
    return reads


class Case:
    """The input, the oracle's reads2 over it and the targets (computed once, never changed)."""

    def __init__(self):
        self.reads = made_reads()
        self.oracle = _pipeline.SplitWindowQ(_pipeline.OracleBackend(), Q)
        self.total_bases = sum(len(s) for _, s, _ in self.reads)
        scored = self.oracle.score(self.reads, PKW, None)
        self.wholly = np.array([r["first"] < 0 for r in scored])
        lengths = np.array([len(s) for _, s, _ in self.reads], dtype=np.int32)
        self.sc = {"mean_q": np.array([r["mean_q"] for r in scored]), "window_q": np.array([r["window_q"] for r in scored]),
                   "passed": np.array([r["passed"] for r in scored], dtype=np.uint8),
                   "child_offsets": np.concatenate([[0], np.cumsum([len(r["children"]) for r in scored])]).astype(np.uint64),
                   "child_ranges": np.array([x for r in scored for x in r["child_ranges"]], dtype=np.int32).reshape(-1, 2),
                   "child_mean_q": np.array([c["mean_q"] for r in scored for c in r["children"]]),
                   "child_window_q": np.array([c["window_q"] for r in scored for c in r["children"]]),
                   "child_passed": np.array([c["passed"] for r in scored for c in r["children"]], dtype=np.uint8)}
        self.lengths = lengths
        self.r2 = _oracle.reads2_gather(lengths, self.sc)
        self.r2_bases = int(self.r2["length"].astype(np.int64).sum())
        self.passed_bases = int(self.r2["length"].astype(np.int64)[self.r2["passed"] != 0].sum())
        self.targets = [int(self.r2_bases * f) for f in np.linspace(0.05, 0.95, 12)]

    def tie_groups(self, lw=1.0):
        """[(bases of the passing entries with a better score, bases of the group, its longest member)] for every group of two or
        more passing CHILDREN with bit-equal final scores (the oracle's scores)."""
        r2 = self.r2
        fs = _oracle.rank_and_cut(r2["mean_q"], r2["window_q"], r2["length"], r2["passed"], lw=lw, target_bases=self.total_bases,
                                  total_bases=self.total_bases)["final_score"]
        ok = r2["passed"] != 0
        ln = r2["length"].astype(np.int64)
        groups = []
        for score in np.unique(fs[ok]):
            members = np.flatnonzero(ok & (fs == score))
            if len(members) >= 2 and (r2["child"][members] >= 0).all():
                groups.append((int(ln[ok & (fs > score)].sum()), int(ln[members].sum()), int(ln[members].max())))
        return groups

    def cuts_a_tie(self, target, lw=1.0):
        """The walk reaches `target` inside a group and leaves a member out whatever the order inside the group is: which member is
        the sort's decision."""
        return any(before < target <= before + total - longest for before, total, longest in self.tie_groups(lw))


@pytest.fixture(scope="module")
def case():
    return Case()


@pytest.fixture(scope="module", params=["select", "sort"])
def hip(request):
    """Both device implementations of the cut, as in test_gpu_rank.py."""
    if request.param == "sort":
        os.environ["FLX_RANK_SORT"] = "1"
    else:
        os.environ.pop("FLX_RANK_SORT", None)
    c = api.Context(0)
    yield _pipeline.SplitWindowQ(_pipeline.HipBackend(c), Q)
    c.close()
    os.environ.pop("FLX_RANK_SORT", None)


def both(case, hip, **kw):
    want = _pipeline.run_filter(case.oracle, case.reads, None, PKW, **kw)
    got = _pipeline.run_filter(hip, case.reads, None, PKW, **kw)
    assert got == want, "%r: names %s, the rest %r / %r" % (kw, "equal" if got[0] == want[0] else "differ", got[1:], want[1:])
    return want, hip.last_report


def test_the_input(case):
    """Conditions on the input, on the oracle alone."""
    r2 = case.r2
    assert case.r2_bases < case.total_bases and len(r2["length"]) > len(case.reads)
    assert case.wholly.sum() >= 20
    for i in np.flatnonzero(case.wholly):  # a wholly bad read stays one failing reads2 entry
        assert list(r2["passed"][(r2["parent"] == i) & (r2["child"] < 0)]) == [0] and not (r2["parent"][r2["child"] >= 0] == i).any()
    assert any(case.cuts_a_tie(t) for t in case.targets), "no target of the grid falls inside a tie group of children"


def test_reads2_of_children(case, hip):
    """flx_reads2_gather over the library's own children against the oracle's over the model's."""
    scored = hip.score(case.reads, PKW, None)
    assert [r["child_ranges"] for r in scored] == [[tuple(x) for x in case.sc["child_ranges"][int(a):int(b)]]
                                                   for a, b in zip(case.sc["child_offsets"][:-1], case.sc["child_offsets"][1:])]
    got = hip.ctx.reads2_gather(case.lengths, case.sc)
    for key in ("mean_q", "window_q"):
        assert (got[key].view(np.uint64) == case.r2[key].view(np.uint64)).all(), key
    for key in ("length", "passed", "parent", "child"):
        assert (got[key] == case.r2[key]).all(), key
    bad = np.flatnonzero(case.wholly)
    assert len(bad) and all(int(got["passed"][(got["parent"] == i) & (got["child"] < 0)][0]) == 0 for i in bad)


def test_targets_across_tie_groups(case, hip):
    fallbacks, child_names = 0, 0
    for t in case.targets:
        want, rep = both(case, hip, target_bases=t)
        # (the last fractions lie above the bases that pass: "already below", on both sides)
        assert want[5] == (api.CUT_SORTED if t < case.passed_bases else api.CUT_ALREADY_BELOW)
        assert want[1] == len(case.r2["length"]) and want[2] == case.r2_bases and want[3] == t
        fallbacks += rep.exact_fallback
        child_names += sum(1 for n in want[0] if CHILD_NAME.search(n))
    assert fallbacks > 0, "no target needed the reference's own sort order"
    assert child_names > 0


def test_keep_percent_weights_and_outcomes(case, hip):
    want, _ = both(case, hip, keep_percent=42.5)
    assert want[3] == int(0.425 * case.total_bases) and want[5] == api.CUT_SORTED  # (of the INPUT's bases)
    both(case, hip, keep_percent=80.0, target_bases=case.r2_bases // 3, lw=2.0, mw=0.5, ww=3.0)
    both(case, hip, target_bases=case.r2_bases // 2, lw=0.0)
    want, _ = both(case, hip, target_bases=case.total_bases)
    assert want[5] == api.CUT_NOT_ENOUGH
    want, _ = both(case, hip, target_bases=case.r2_bases + 1)  # more than reads2 holds, less than the input: not "not enough"
    assert want[5] == api.CUT_ALREADY_BELOW and case.r2_bases + 1 < case.total_bases
    want, _ = both(case, hip, target_bases=case.passed_bases)
    assert want[5] == api.CUT_ALREADY_BELOW
    want, _ = both(case, hip, target_bases=case.passed_bases - 1)  # just under what passes: the cut is made
    assert want[5] == api.CUT_SORTED
    want, _ = both(case, hip)
    assert want[5] == api.CUT_NONE and any(CHILD_NAME.search(n) for n in want[0])


def test_sharded_select_over_children(case):
    """The same reads2 arrays over three ranks on one GPU: the pass set of the one-rank stage (check_out holds every rank's slice
    against the oracle; where the ranks hand the decision back, the flags are untouched and the one-rank stage decides)."""
    os.environ.pop("FLX_RANK_SORT", None)
    r2 = case.r2
    mean, window = np.ascontiguousarray(r2["mean_q"]), np.ascontiguousarray(r2["window_q"])
    length, passed = np.ascontiguousarray(r2["length"]), np.ascontiguousarray(r2["passed"])
    ctx = api.Context(0)
    try:
        decided = 0
        for t in (case.targets[1], case.targets[6], case.targets[10]):
            kw = dict(target_bases=t, total_bases=case.total_bases)
            one = ctx.rank_and_cut(mean, window, length, passed, **kw)
            want = _oracle.rank_and_cut(mean, window, length, passed, **kw)
            assert (one["passed"] == want["passed"]).all()
            res, _, out = check_out(even(len(mean), 3), mean, window, length, passed, **kw)
            if res == "ok":
                decided += 1
                assert (np.concatenate([o[0] for o in out]) == one["passed"]).all()
        assert decided > 0
    finally:
        ctx.close()
