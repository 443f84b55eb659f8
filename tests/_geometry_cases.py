"""Batches sized by the LAUNCH GEOMETRY of the Phred-mode stack (--trim_adapters, --exclude, the children of flx_phred_children), not
by their content: how many read ends a workgroup of k_adapter_cuts takes, how many spans a wave of k_screen_hits walks, where the
sentinel of an n + 1-element kernel and the tiles of the scans and of the radix sort end.  tests/test_geometry_cases.py holds every
batch against the conditions it was built for, on the models and the formulas mirrored here alone; the three *_geometry_gpu.py files
run them.

The numbers below MIRROR constants of the kernels; source_constants() reads the originals out of the sources, and the CPU test
compares, so that a retuned kernel fails a test without a GPU instead of silently losing its coverage."""
import functools
import os
import re

import numpy as np

import _adapters_cases as cases
import _adapters_model as amodel
import _screen_model as smodel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MIRRORED = {  # name in the source: (file under filtlong_amd/csrc, value)
    "kThreads": ("adapters.hip", 256), "kItemsPerGroup": ("adapters.hip", 1024), "kLdsTextBytes": ("adapters.hip", 32768),
    "kMaxEnds": ("adapters.hip", 1024), "kScreenThreads": ("screen.hip", 1024), "kScreenSpan": ("screen.h", 4096),
    "SCAN_THREADS": ("sort.hip", 256), "SCAN_ITEMS": ("sort.hip", 8), "RS_ROUNDS": ("sort.hip", 16), "RS_WAVES": ("sort.hip", 4),
}
K_THREADS = MIRRORED["kThreads"][1]
SCREEN_WAVES = MIRRORED["kScreenThreads"][1] // 64                      # waves per workgroup of k_screen_hits
SCREEN_SPAN = MIRRORED["kScreenSpan"][1]
SCAN_TILE = MIRRORED["SCAN_THREADS"][1] * MIRRORED["SCAN_ITEMS"][1]     # sort.hip: SCAN_TILE = SCAN_THREADS * SCAN_ITEMS
RS_TILE = 64 * MIRRORED["RS_ROUNDS"][1]                                 # sort.hip: RS_TILE = 64 * RS_ROUNDS, keys per wave
RS_BLOCK = RS_TILE * MIRRORED["RS_WAVES"][1]                            # keys per workgroup of k_radix_hist / k_radix_scatter
SENTINEL_BLOCK = 256                                                    # the n + 1-element kernels launch (n + 1 + 255) / 256 blocks


def groups_of(P, W):
    """read ends per workgroup of k_adapter_cuts (`epb`) for P patterns and --adapter_window W: mirrors kItemsPerGroup, kLdsTextBytes
    and kMaxEnds of csrc/adapters.hip (flx_adapter_cuts_dev)"""
    stride = (W + 15) & ~15
    return max(1, min(MIRRORED["kItemsPerGroup"][1] // P, MIRRORED["kLdsTextBytes"][1] // stride, MIRRORED["kMaxEnds"][1]))


def source_constants():
    """the values the sources give the mirrored names today: {name: int}"""
    out = {}
    for name, (fname, _) in MIRRORED.items():
        text = open(os.path.join(ROOT, "filtlong_amd", "csrc", fname)).read()
        m = re.search(r"constexpr\s+int\s+%s\s*=\s*([^;]+);" % name, text)
        assert m, (name, fname)
        expr = m.group(1).strip()
        assert re.fullmatch(r"[0-9 <*+()]+", expr), (name, expr)  # digits and shifts only: 1 << 15 style
        out[name] = int(eval(expr))
    return out


def arrange(proc, order):
    """the reads in INPUT order such that the read processed at place i (order[i]) is proc[i]"""
    inp = [None] * len(proc)
    for place, r in enumerate(order):
        inp[int(r)] = proc[place]
    return inp


# ---- adapters ------------------------------------------------------------------------------------------------------------------------
# (name, sequences, W, epb, pattern lengths, E, class).  P = 2 * sequences.  The many-pattern sets have long patterns of one or two
# lengths and E = 10: a random 1024-base text holds no 40-mer within 4 edits, while 256 12-mers within 2 edits would hit every read.
ADAPTER_CASES = [
    ("p2_w16", 1, 16, 512, (12,), 20, "second staging round"),
    ("p2_w64", 1, 64, 512, (28,), 20, "LDS limit and item limit coincide"),
    ("p2_w65", 1, 65, 409, (28,), 20, "odd, LDS-bound, above 256"),
    ("p4_w16", 2, 16, 256, (12, 13), 20, "exactly one staging round"),
    ("p2_w150", 1, 150, 204, (28,), 20, "the default window"),
    ("p6_w150", 3, 150, 170, (28, 12, 16), 20, "item-bound, several groups"),
    ("p2_w1024", 1, 1024, 32, (28,), 20, "LDS-bound, several groups"),
    ("p64_w1024", 32, 1024, 16, (40, 48), 10, "item-bound at the widest window"),
    ("p256_w1024", 128, 1024, 4, (40,), 10, "the smallest epb"),
]
ADAPTER_KINDS = ("partial", "multiple", "below")  # >= 3 workgroups, the last partial | n_ends a multiple of epb | n_ends < epb


def adapter_case(name):
    return next(c for c in ADAPTER_CASES if c[0] == name)


def adapter_seqs(case):
    name, n_seqs, w, _, lens, _, _ = case
    rng = np.random.default_rng(1000 + ADAPTER_CASES.index(case))
    return [cases.LIGATION if m == 28 else cases.random_adapter(rng, m) for m in (lens[i % len(lens)] for i in range(n_seqs))]


def adapter_reads_of(epb, kind):
    if kind == "partial":
        return epb + epb // 16 + 3   # 2 epb + epb / 8 + 6 ends: two full workgroups and a part of a third
    if kind == "multiple":
        return epb                   # 2 epb ends: two full workgroups (an odd epb splits the middle read between them)
    return max(1, (epb - 1) // 2)    # the most ends below epb: one partial workgroup


@functools.lru_cache(maxsize=None)
def adapter_pool(name):
    """the distinct reads of a case by what they are MEANT to be (the model decides what they are): head / tail hold an adapter at
    that end only.  One pool per case, whatever the batch: the model is asked once per distinct text (KEY_CACHE)"""
    case = adapter_case(name)
    seqs, w = adapter_seqs(case), case[2]
    rng = np.random.default_rng(3000 + ADAPTER_CASES.index(case))
    a = bytes(seqs[0]).upper()
    m = len(a)
    others = [bytes(seqs[-1]).upper(), amodel.revcomp(bytes(seqs[len(seqs) // 2]).upper())]
    big = 2 * w + 40
    body = lambda n: cases.random_seq(rng, max(n, 0))
    offs = [o for o in (0, 1, 2, 3) if o + m <= w]
    pool = {"head": [], "tail": [], "both": [], "none": []}
    for o in offs:
        pool["head"].append(body(o) + a + body(big))
        pool["tail"].append(body(big) + amodel.revcomp(a) + body(o))
    for k in (1, 2):  # 1 and 2 substitutions
        pool["head"].append(cases.substitute(rng, a, k) + body(big))
        pool["tail"].append(body(big) + cases.substitute(rng, a, k))
    for x in others:
        if len(x) <= w:
            pool["head"].append(x + body(big))
            pool["tail"].append(body(big) + x)
    pool["head"].append(a + body(1030))                                # at least 1024 bases: a 128-byte start
    pool["tail"].append(body(1100) + amodel.revcomp(a))
    pool["both"].append(a + body(big) + amodel.revcomp(a))
    pool["both"].append(body(offs[-1]) + a + body(big) + a + body(offs[-1]))
    pool["both"].append(cases.substitute(rng, a, 1) + body(1040) + others[0])
    for n in (0, 1, w - 1, w, w + 7, big, 1030):                        # lengths 0, 1, below W, W, above W, at least 1024
        pool["none"].append(body(n))
    return pool


def adapter_batch(name, kind):
    """(seqs, W, E, epb, reads in PROCESSING order).  Both sides of every workgroup boundary are meant to hold a hit, every workgroup a
    hit and a miss: read b / 2 - 1 ends in a tail hit and read b / 2 starts with a head hit at an even boundary b (in ends), the read
    that straddles an odd boundary carries both."""
    case = adapter_case(name)
    _, n_seqs, w, epb, _, errors, _ = case
    seqs = adapter_seqs(case)
    rng = np.random.default_rng(7000 + 10 * ADAPTER_CASES.index(case) + ADAPTER_KINDS.index(kind))
    pool = adapter_pool(name)
    n = adapter_reads_of(epb, kind)
    proc = [None] * n
    took = {"head": 0, "tail": 0, "both": 0}

    def take(what):
        took[what] += 1
        return pool[what][(took[what] - 1) % len(pool[what])]
    proc[0] = take("head")
    for b in range(epb, 2 * n, epb):
        if b % 2 == 0:
            proc[b // 2 - 1], proc[b // 2] = take("tail"), take("head")
        else:
            proc[b // 2] = take("both")
    every = [r for what in ("none", "head", "both", "tail") for r in pool[what]]
    every = [every[i] for i in rng.permutation(len(every))]
    free = [i for i in range(n) if proc[i] is None]
    for k, i in enumerate(free):
        proc[i] = every[k % len(every)]
    return seqs, w, errors, epb, proc


KEY_CACHE = {}  # case name -> {(side, text): key}


def adapter_keys(name, reads):
    case = adapter_case(name)
    return keys_by_text(reads, case[2], amodel.patterns(adapter_seqs(case)), case[5], KEY_CACHE.setdefault(name, {}))


def keys_by_text(reads, window, pats, errors, cache=None):
    """model.keys_of, one end_key per DISTINCT text: an end's key depends on the W bases at that end alone"""
    cache = {} if cache is None else cache
    out = np.zeros((len(reads), 2), dtype=np.uint32)
    for i, r in enumerate(reads):
        r = bytes(r)
        for side, text in ((0, r[:window]), (1, r[-window:] if r else b"")):
            if (side, text) not in cache:
                cache[(side, text)] = amodel.end_key(text, side, window, pats, errors)
            out[i, side] = cache[(side, text)]
    return out


# ---- the screen ------------------------------------------------------------------------------------------------------------------------
def spans_of(reads, span=SCREEN_SPAN):
    return np.array([(max(0, len(r) - 15) + span - 1) // span for r in reads], dtype=np.int64)


def crowd_reads(n_cu):
    """reads of a crowd that gives every wave of the widest grid (2 n_cu workgroups of SCREEN_WAVES waves) 2.5 spans: about one span a
    read, some 7 % of the reads have none"""
    return int(2.5 * 2 * n_cu * SCREEN_WAVES * 1.08) + 64


def from_ref(rng, ref, length, rate):
    """a read of any length from a short reference: fragments of it, either strand, one after the other"""
    out = b""
    while len(out) < length:
        out += smodel.draw(rng, ref, min(len(ref), length - len(out), 3000), rate)
    return out


def crowd(ref, n_reads, seed, span=SCREEN_SPAN):
    """(reads in PROCESSING order, places): mostly reads of 16 to 80 bases (one span each) drawn from `ref` clean, with 5 %
    substitutions, or unrelated; reads of span + 15, 2 span + 16 and 40 000 bases at the start, in the middle and at the end; reads
    below 16 bases (no span) alone and in runs, the first three and the last three among them"""
    assert n_reads >= 200
    rng = np.random.default_rng(seed)
    lens = rng.integers(16, 81, size=n_reads)
    what = rng.integers(0, 4, size=n_reads)
    unrelated = smodel.random_seq(rng, 100 * n_reads)
    reads = []
    for i in range(n_reads):
        n = int(lens[i])
        if what[i] == 0:
            reads.append(smodel.draw(rng, ref, n))
        elif what[i] == 1:
            reads.append(smodel.draw(rng, ref, n, 0.05))
        else:
            reads.append(unrelated[100 * i:100 * i + n])
    places = {"none": [0, 1, 2, n_reads - 3, n_reads - 2, n_reads - 1], "long": {}}
    for at in rng.integers(10, n_reads // 3 - 10, size=8):              # single ones (clear of the runs and of the long reads)
        places["none"].append(int(at))
    for at, run in ((n_reads // 3, 5), (2 * n_reads // 3, 40)):          # runs
        places["none"] += list(range(at, at + run))
    for k, at in enumerate(places["none"]):
        reads[at] = smodel.draw(rng, ref, (0, 1, 15, 7)[k % 4])
    for where, at in (("start", 3), ("middle", n_reads // 2), ("end", n_reads - 6)):
        places["long"][where] = [at, at + 1, at + 2]
        for k, n in enumerate((span + 15, 2 * span + 16, 40000)):
            reads[at + k] = from_ref(rng, ref, n, 0.05 if k else 0.0)
    return reads, places


# ---- the children ----------------------------------------------------------------------------------------------------------------------
# One exact adapter at the head (E = 0, W = the adapter's length): a read `adapter + body` has the one child [28, 28 + len(body)), so
# child lengths are chosen exactly.  Every body is a SUFFIX of one filler, so the tails repeat and the model is asked once per text.
CHILD_ADAPTER = cases.LIGATION
CHILD_W = len(CHILD_ADAPTER)
CHILD_E = 0
_FILLER = cases.random_seq(np.random.default_rng(99), 60000)
_WHOLE = [b"", b"A", _FILLER[100:120], _FILLER[200:300], _FILLER[1000:2030], _FILLER[3000:3015]]  # no adapter: no cut, no child

CHILD_COUNTS = (1, 2, RS_TILE - 1, RS_TILE, RS_TILE + 1, RS_BLOCK - 1, RS_BLOCK, RS_BLOCK + 1)
CHILD_BATCHES = [  # (child count, length class): the sort passes are those of the class
    (1, "one"), (2, "byte"), (RS_TILE - 1, "byte"), (RS_TILE, "one"), (RS_TILE + 1, "wide"), (RS_BLOCK - 1, "byte"),
    (RS_BLOCK, "one"), (RS_BLOCK + 1, "byte"), (RS_BLOCK + 1, "wide"), (300, "few_long"),
]
SORT_PASSES = {"one": 0, "byte": 1, "wide": 2, "few_long": 2}
READ_COUNTS = (255, 256, 257, 511, 512, SCAN_TILE - 1, SCAN_TILE)
READ_BATCHES = [(n, share) for n in READ_COUNTS for share in ("none", "some", "all")]


def child_lengths(rng, nc, cls):
    if cls == "one":
        return np.full(nc, 137, dtype=np.int64)
    if cls == "byte":       # within one low byte of the key 0x7fffffff - length: exactly one sort pass
        out = rng.integers(1, 256, size=nc)
        out[:2] = (1, 255)[:nc]
    elif cls == "wide":     # 1 .. 60 000: two passes
        out = rng.integers(1, 2001, size=nc)
        edge = np.array([1, 255, 256, 1023, 1024, 1025, 30000, 60000])
        out[rng.choice(nc, size=len(edge), replace=False)] = edge
    else:                   # few_long: 128-byte child slots among 16-byte ones, gaps in the child plane
        out = rng.integers(1, 200, size=nc)
        edge = np.array([1024, 1025, 1500, 3000, 1024])
        out[rng.choice(nc - 2, size=len(edge), replace=False) + 1] = edge
    return out.astype(np.int64)


def sort_passes(lengths):
    """the passes flx_radix_sort_pairs runs on the keys 0x7fffffff - length: one per key byte that is not constant"""
    if len(lengths) <= 1:
        return 0
    keys = 0x7fffffff - np.asarray(lengths, dtype=np.int64)
    varying = int(np.bitwise_or.reduce(keys)) & ~int(np.bitwise_and.reduce(keys))
    return sum(1 for b in range(8) if (varying >> (8 * b)) & 0xff)


def child_read(cl, tail_too=False):
    """a read whose one child has `cl` bases; tail_too: the adapter's reverse complement at the tail is cut off as well"""
    assert 0 < cl <= len(_FILLER)
    return CHILD_ADAPTER + _FILLER[len(_FILLER) - cl:] + (amodel.revcomp(CHILD_ADAPTER) if tail_too else b"")


def quals_for(rng, reads):
    """quality strings of the reads' lengths: a level per read (Q 2 .. 29) and a little noise, so that min_mean_q parts them"""
    out = []
    for r in reads:
        level = int(rng.integers(2, 30))
        out.append((33 + level + rng.integers(0, 5, size=len(r))).astype(np.uint8).tobytes())
    return out


def _with_childless(rng, kids, n_other, last_has_child):
    """the reads with a child and n_other reads without one (the adapter alone: nothing left; no adapter: nothing cut), shuffled; the
    designed child length of every read (0: no child)"""
    other = [CHILD_ADAPTER if k % 2 == 0 else _WHOLE[(k // 2) % len(_WHOLE)] for k in range(n_other)]
    reads = [(r, cl) for r, cl in kids] + [(r, 0) for r in other]
    reads = [reads[i] for i in rng.permutation(len(reads))]
    has = [i for i, (_, cl) in enumerate(reads) if cl]
    lacks = [i for i, (_, cl) in enumerate(reads) if not cl]
    want_last = has if last_has_child else lacks
    if want_last and (reads[-1][1] > 0) != last_has_child:
        i = want_last[-1]
        reads[i], reads[-1] = reads[-1], reads[i]
    return [r for r, _ in reads], np.array([cl for _, cl in reads], dtype=np.int64)


def children_batch(nc, cls, seed=0):
    """(reads, quals, designed child length per read): nc children of the class's lengths, a few reads without a child among them"""
    rng = np.random.default_rng(50000 + 16 * nc + seed + sum(map(ord, cls)))
    lens = child_lengths(rng, nc, cls)
    kids = [(child_read(int(cl), tail_too=(k % 7 == 3)), int(cl)) for k, cl in enumerate(lens)]
    reads, designed = _with_childless(rng, kids, max(3, nc // 64), last_has_child=nc % 2 == 1)
    return reads, quals_for(rng, reads), designed


def reads_batch(n_reads, share, seed=0):
    """n_reads reads of which none, some (about half, the last one among them) or all have a child"""
    rng = np.random.default_rng(60000 + 4 * n_reads + seed + len(share))
    nc = {"none": 0, "some": n_reads // 2, "all": n_reads}[share]
    lens = child_lengths(rng, nc, "few_long" if nc >= 100 else "byte") if nc else []
    kids = [(child_read(int(cl), tail_too=(k % 5 == 1)), int(cl)) for k, cl in enumerate(lens)]
    reads, designed = _with_childless(rng, kids, n_reads - nc, last_has_child=nc > 0)
    return reads, quals_for(rng, reads), designed


def children_of(reads, cache=None):
    """by the model: (keys, [(parent, s, e)] in read order)"""
    keys = keys_by_text(reads, CHILD_W, amodel.patterns([CHILD_ADAPTER]), CHILD_E, cache)
    kids = []
    for i, r in enumerate(reads):
        for s, e in amodel.child_of(len(r), keys[i, 0], keys[i, 1])[0]:
            kids.append((i, s, e))
    return keys, kids
