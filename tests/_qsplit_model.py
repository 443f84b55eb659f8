"""--split_window_q, written from its definition (include/filtlong_hip.h, csrc/qsplit.h) and from nothing else: the error table
from 60-digit decimals, the threshold from the one double expression, the bad windows from a cumulative sum and the children as
the maximal runs of the bases no bad window covers.  Shared by the CPU and the GPU tests; not a test module."""
import struct
from decimal import ROUND_FLOOR, Decimal, getcontext

import numpy as np

U32_MAX = 2 ** 32 - 1


def error_table():
    getcontext().prec = 60
    e = []
    for b in range(256):
        q = (b - 256 if b >= 128 else b) - 33
        if q <= 0:
            e.append(U32_MAX)
        else:
            x = Decimal(10) ** (Decimal(-q) / Decimal(10)) * Decimal(2 ** 32) + Decimal("0.5")
            e.append(min(U32_MAX, int(x.to_integral_value(rounding=ROUND_FLOOR))))
    return e


E = np.array(error_table(), dtype=np.uint64)


def threshold(q):
    return int(np.floor((100.0 - float(q)) / 100.0 * 4294967296.0))


def children(qual, w, t):
    """qual: bytes.  Returns (ranges [(start, end)], first, last, any_bad): the children are the maximal runs of bases that lie
    in no bad window; the window ending at j (n - 1 <= j < L, n = min(w, L)) is bad iff its sum of E is > t * n."""
    L = len(qual)
    if L == 0:
        return [], 0, 0, False
    n = min(w, L)
    assert L < 2 ** 31 and t * n < 2 ** 64  # (every sum then fits uint64)
    c = np.concatenate((np.zeros(1, dtype=np.uint64), np.cumsum(E[np.frombuffer(qual, dtype=np.uint8)], dtype=np.uint64)))
    sums = c[n:] - c[:-n]  # sums[k]: the window ending at j = n - 1 + k
    bad_ends = np.flatnonzero(sums > np.uint64(t * n)) + (n - 1)
    if len(bad_ends) == 0:
        return [], 0, L, False
    # removed[i]: base i lies in a bad window [j - n + 1, j]  (difference array)
    d = np.zeros(L + 1, dtype=np.int64)
    np.add.at(d, bad_ends - (n - 1), 1)
    np.add.at(d, bad_ends + 1, -1)
    kept = np.cumsum(d[:L]) == 0
    edges = np.flatnonzero(np.diff(np.concatenate(([0], kept.astype(np.int8), [0]))))
    ranges = [(int(edges[k]), int(edges[k + 1])) for k in range(0, len(edges), 2)]
    if not ranges:
        return [], -1, -1, True
    return ranges, ranges[0][0], ranges[-1][1], True


def split_batch(quals, w, q):
    """The child CSR of a batch: (child_offsets, child_ranges [nc, 2], first, last, wholly_bad mask)."""
    t = threshold(q)
    off, rng, first, last, wholly = [0], [], [], [], []
    for s in quals:
        r, f, l, any_bad = children(s, w, t)
        rng += r
        off.append(len(rng))
        first.append(f)
        last.append(l)
        wholly.append(any_bad and not r)
    return (np.array(off, dtype=np.uint64), np.array(rng, dtype=np.int32).reshape(-1, 2), np.array(first, dtype=np.int32),
            np.array(last, dtype=np.int32), np.array(wholly, dtype=bool))


def census(child_offsets, wholly):
    """How a batch split: reads with at least 2 children, wholly bad reads, untouched reads (no child, not wholly bad)."""
    per = np.diff(child_offsets.astype(np.int64))
    return int((per >= 2).sum()), int(wholly.sum()), int(((per == 0) & ~wholly).sum())


def junk_read(rng, length, stretches, good=(12, 34), junk=(1, 5)):
    """A quality string of Phred good[0]..good[1] with the half-open `stretches` at Phred junk[0]..junk[1]."""
    q = rng.integers(good[0], good[1] + 1, size=length)
    for a, b in stretches:
        a, b = max(0, a), min(length, b)
        if b > a:
            q[a:b] = rng.integers(junk[0], junk[1] + 1, size=b - a)
    return (q + 33).astype(np.uint8).tobytes()


def pack_cases(cases):
    """[(w, t, qual)] in the form tests/qsplit_host.cpp reads."""
    out = [struct.pack("<I", len(cases))]
    for w, t, s in cases:
        out.append(struct.pack("<qQQ", w, t, len(s)) + s)
    return b"".join(out)
