"""The batches of tests/_geometry_cases.py are what the *_geometry_gpu.py tests take them for — checked on the models and the mirrored
formulas alone, without a GPU.  A batch exists to reach one loop round or branch of a kernel; whether it does depends on constants
of that kernel (kItemsPerGroup, kLdsTextBytes, kMaxEnds, kThreads of csrc/adapters.hip; kScreenThreads, kScreenSpan of the screen;
SCAN_TILE, RS_TILE, RS_WAVES of csrc/sort.hip).  If one of them is retuned, a test here fails, on a CPU, instead of the coverage
vanishing silently: the mirrored values are compared with the sources, and every class is asserted on the mirrored formula."""
import numpy as np
import pytest

import _adapters_model as amodel
import _geometry_cases as geo
import _screen_model as smodel


def test_mirrored_constants_are_the_sources():
    assert geo.source_constants() == {name: value for name, (_, value) in geo.MIRRORED.items()}
    assert (geo.SCAN_TILE, geo.RS_TILE, geo.RS_BLOCK, geo.SCREEN_WAVES, geo.SCREEN_SPAN) == (2048, 1024, 4096, 16, 4096)


# ---- adapters ------------------------------------------------------------------------------------------------------------------------
def test_every_epb_class_is_hit():
    epb = {name: geo.groups_of(2 * n_seqs, w) for name, n_seqs, w, _, _, _, _ in geo.ADAPTER_CASES}
    for name, n_seqs, w, want, _, _, _ in geo.ADAPTER_CASES:
        assert epb[name] == want, (name, epb[name], want)
    lds = lambda w: geo.MIRRORED["kLdsTextBytes"][1] // ((w + 15) & ~15)
    items = lambda p: geo.MIRRORED["kItemsPerGroup"][1] // p
    t = geo.K_THREADS
    assert epb["p2_w16"] == 2 * t and items(2) < lds(16)               # a second staging round, full; item-bound
    assert epb["p2_w64"] > t and items(2) == lds(64)                   # the two limits coincide
    assert t < epb["p2_w65"] < 2 * t and epb["p2_w65"] % 2 == 1 and lds(65) < items(2)  # odd, LDS-bound, a partial second round
    assert epb["p4_w16"] == t                                          # exactly one staging round
    assert epb["p2_w150"] < t and lds(150) < items(2)                  # the default window: LDS-bound
    assert epb["p6_w150"] < t and items(6) < lds(150)                  # item-bound
    assert epb["p2_w1024"] == lds(1024) < items(2)                     # LDS-bound at the widest window
    assert epb["p64_w1024"] == items(64) < lds(1024)
    assert epb["p256_w1024"] == items(256) == 4                        # the smallest epb: 256 patterns are the most a set has
    assert 2 * amodel.MAX_SEQS == 256


@pytest.mark.parametrize("kind", geo.ADAPTER_KINDS)
@pytest.mark.parametrize("name", [c[0] for c in geo.ADAPTER_CASES])
def test_adapter_batches(name, kind):
    seqs, w, errors, epb, proc = geo.adapter_batch(name, kind)
    assert epb == geo.groups_of(2 * len(seqs), w)
    ends = geo.adapter_keys(name, proc).reshape(-1)  # end 2 i the head, 2 i + 1 the tail of the read processed at place i
    n_ends = len(ends)
    groups = (n_ends + epb - 1) // epb
    if kind == "partial":
        assert groups >= 3 and n_ends % epb != 0
    elif kind == "multiple":
        assert groups >= 2 and n_ends % epb == 0
    else:
        assert n_ends < epb and 2 * (len(proc) + 1) >= epb
    for g in range(groups):  # every workgroup's ends hold a hit and a miss
        seg = ends[g * epb:(g + 1) * epb]
        assert (seg > 0).any() and (seg == 0).any(), (name, kind, g)
    for b in range(epb, n_ends, epb):  # both sides of every boundary hold a hit
        assert ends[b - 1] > 0 and ends[b] > 0, (name, kind, b)
    if epb > geo.K_THREADS:  # the second staging round holds real reads, with hits: the local ends from kThreads on of a workgroup
        late = np.concatenate([ends[g * epb + geo.K_THREADS:(g + 1) * epb] for g in range(groups)])
        assert (late > 0).sum() >= 3 and (late == 0).sum() >= 3
    if epb % 2 == 1 and kind != "below":  # a read with its head and its tail in different workgroups, and both hit
        split = [i for i in range(len(proc)) if (2 * i) // epb != (2 * i + 1) // epb]
        assert split and all(ends[2 * i] > 0 and ends[2 * i + 1] > 0 for i in split)
    if len(proc) >= 30:  # the mix: lengths 0, 1, below W, W, above W, at least 1024; 1 and 2 substitutions are in the pool
        lens = {len(r) for r in proc}
        assert {0, 1, w} <= lens and any(1 < n < w for n in lens) and any(w < n < w + 16 for n in lens) and any(n >= 1024 for n in lens)
        hit = ends.reshape(-1, 2) > 0
        assert (hit[:, 0] & ~hit[:, 1]).any() and (~hit[:, 0] & hit[:, 1]).any() and hit.all(axis=1).any() and (~hit.any(axis=1)).any()
        assert len(set(ends.tolist())) >= 5  # several different keys: neighbours are told apart


def test_some_read_has_head_and_tail_in_different_workgroups():
    found = []
    for name, _, _, epb, _, _, _ in geo.ADAPTER_CASES:
        for kind in ("partial", "multiple"):
            n = geo.adapter_reads_of(epb, kind)
            found += [(name, kind, i) for i in range(n) if (2 * i) // epb != (2 * i + 1) // epb]
    assert found and {f[0] for f in found} == {"p2_w65"}


def test_keys_by_text_is_keys_of():
    seqs, w, errors, _, proc = geo.adapter_batch("p4_w16", "below")
    pats = amodel.patterns(seqs)
    assert (geo.keys_by_text(proc, w, pats, errors) == amodel.keys_of(proc, w, pats, errors)).all()
    reads, _, _ = geo.children_batch(2, "byte")
    pats = amodel.patterns([geo.CHILD_ADAPTER])
    assert (geo.keys_by_text(reads, geo.CHILD_W, pats, geo.CHILD_E) == amodel.keys_of(reads, geo.CHILD_W, pats, geo.CHILD_E)).all()


def test_arrange_puts_the_batch_into_processing_order():
    proc = [bytes([65 + i]) for i in range(7)]
    order = np.random.default_rng(1).permutation(7)
    inp = geo.arrange(proc, order)
    assert [inp[int(r)] for r in order] == proc


# ---- the screen ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ref5k():
    return smodel.random_seq(np.random.default_rng(101), 5000)


@pytest.mark.parametrize("n_cu", [8, 256, 304])
def test_crowd_gives_every_wave_two_spans_and_some_three(ref5k, n_cu):
    n = geo.crowd_reads(n_cu)
    reads, places = geo.crowd(ref5k, n, 5)
    spans = geo.spans_of(reads)
    start = np.concatenate(([0], np.cumsum(spans)))
    assert len(reads) == n
    for blocks in (n_cu, 2 * n_cu):  # the LDS form, and the pre12 and exact forms
        waves = blocks * geo.SCREEN_WAVES
        assert start[-1] >= 2.5 * waves  # every wave takes two spans, half of them three
        rounds = {where: {int(start[i]) // waves for i in at} for where, at in places["long"].items()}
        assert max(rounds["start"]) == 0 and (int(start[-1]) - 1) // waves >= 2  # (some wave takes a third span)
        assert min(rounds["middle"]) > max(rounds["start"]) and min(rounds["end"]) > max(rounds["middle"])  # different rounds
    assert (spans[:3] == 0).all() and (spans[-3:] == 0).all() and spans[3] > 0 and spans[-4] > 0  # the binary search's edges
    runs, run = [], 0
    for s in spans[3:-3].tolist() + [1]:
        if s == 0:
            run += 1
        elif run:
            runs.append(run)
            run = 0
    assert 1 in runs and any(5 <= r < 40 for r in runs) and max(runs) >= 40  # single ones and runs, away from the batch's ends
    for at in places["long"].values():
        assert [len(reads[i]) for i in at] == [geo.SCREEN_SPAN + 15, 2 * geo.SCREEN_SPAN + 16, 40000]
        assert spans[at].tolist() == [1, 3, 10]
    one = spans == 1
    assert one.mean() > 0.85 and all(16 <= len(reads[i]) <= 80 or i in sum(places["long"].values(), []) for i in np.flatnonzero(one))


@pytest.mark.parametrize("n_reads", [geo.SCAN_TILE - 1, geo.SCAN_TILE, geo.SCAN_TILE + 1])
def test_crowds_at_the_scan_tile(ref5k, n_reads):
    """n_reads + 1 counts go through the u32 scan: 2048 (one full tile), 2049 and 2050 (a second tile of one and two)"""
    reads, places = geo.crowd(ref5k, n_reads, 6)
    spans = geo.spans_of(reads)
    assert len(reads) + 1 in (geo.SCAN_TILE, geo.SCAN_TILE + 1, geo.SCAN_TILE + 2)
    assert (spans[:3] == 0).all() and (spans[-3:] == 0).all() and spans.sum() > n_reads * 0.9


def test_hits_many_is_hits(ref5k):
    x = smodel.build_set([ref5k])
    reads, places = geo.crowd(ref5k, 600, 7)
    reads += [b"", ref5k, ref5k[:16], ref5k[:15], b"N" * 40, ref5k[100:140].lower(), b""]
    got = smodel.hits_many(x, reads)
    want = np.array([smodel.hits(x, r) for r in reads], dtype=np.uint32)
    assert got.dtype == np.uint32 and (got == want).all()
    assert (want > 0).sum() > 100 and (want == 0).sum() > 100 and want[601] == 5000 - 15
    assert smodel.hits_many(x, []).tolist() == [] and smodel.hits_many(x, [b""]).tolist() == [0]


# ---- the children ----------------------------------------------------------------------------------------------------------------------
def test_child_counts_sit_on_the_sort_edges():
    assert geo.CHILD_COUNTS == (1, 2, 1023, 1024, 1025, 4095, 4096, 4097)
    assert {nc for nc, _ in geo.CHILD_BATCHES} >= set(geo.CHILD_COUNTS)
    assert geo.READ_COUNTS == (255, 256, 257, 511, 512, 2047, 2048)
    assert {n % geo.SENTINEL_BLOCK for n in geo.READ_COUNTS} >= {0, 1, geo.SENTINEL_BLOCK - 1}  # the sentinel alone in its block
    assert {n + 1 for n in geo.READ_COUNTS} >= {geo.SCAN_TILE, geo.SCAN_TILE + 1}                # the i64 scan's tile edge


@pytest.fixture(scope="module")
def text_cache():
    return {}


@pytest.mark.parametrize("nc,cls", geo.CHILD_BATCHES)
def test_children_batches(text_cache, nc, cls):
    reads, quals, designed = geo.children_batch(nc, cls)
    assert [len(q) for q in quals] == [len(r) for r in reads]
    keys, kids = geo.children_of(reads, text_cache)
    assert len(kids) == nc
    got = np.zeros(len(reads), dtype=np.int64)
    for parent, s, e in kids:
        assert s == geo.CHILD_W and e > s
        got[parent] = e - s
    assert (got == designed).all()  # the child lengths are the chosen ones
    lens = np.array([e - s for _, s, e in kids])
    assert geo.sort_passes(lens) == geo.SORT_PASSES[cls]
    if cls == "one":
        assert len(set(lens.tolist())) == 1
    elif cls == "byte":
        assert lens.min() == 1 and lens.max() <= 255 and (nc < 2 or lens.max() == 255)
    elif cls == "wide":
        assert lens.min() == 1 and lens.max() == 60000 and {255, 256, 1023, 1024, 1025} <= set(lens.tolist())
    else:
        assert 3 <= (lens >= 1024).sum() <= 8 and (lens < 256).mean() > 0.9 and 1024 in lens and lens[0] < 1024 and lens[-1] < 1024
    firsts = [amodel.child_of(len(r), k[0], k[1])[1] for r, k in zip(reads, keys)]
    assert -1 in firsts and 0 in firsts  # a read with nothing left and a read with nothing cut are among them
    assert (designed[-1] > 0) == (nc % 2 == 1)


@pytest.mark.parametrize("n_reads,share", geo.READ_BATCHES)
def test_reads_batches(text_cache, n_reads, share):
    reads, quals, designed = geo.reads_batch(n_reads, share)
    keys, kids = geo.children_of(reads, text_cache)
    assert len(reads) == n_reads and len(kids) == {"none": 0, "some": n_reads // 2, "all": n_reads}[share]
    got = np.zeros(n_reads, dtype=np.int64)
    for parent, s, e in kids:
        got[parent] = e - s
    assert (got == designed).all()
    assert (designed[-1] > 0) == (share != "none")  # the last read has a child wherever there are children
    if share == "none":
        firsts = {amodel.child_of(len(r), k[0], k[1])[1] for r, k in zip(reads, keys)}
        assert firsts == {-1, 0}
