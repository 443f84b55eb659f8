"""Reads for the --trim_adapters tests: every placement and edge the definition has, at the sizes of one (adapter set, W) pair."""
import numpy as np

import _adapters_model as model

LIGATION = b"AATGTACTTCGTTCAGTTACGTATTGCT"  # 28 bases: the ligation adapter's top strand


def random_seq(rng, n):
    return bytes(np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=n)]) if n else b""


def random_adapter(rng, m):
    return random_seq(rng, m)


def substitute(rng, seq, count):
    s = bytearray(seq)
    for at in rng.choice(len(s), size=count, replace=False):
        s[at] = b"ACGT"[(b"ACGT".index(s[at]) + int(rng.integers(1, 4))) % 4]
    return bytes(s)


def indel(rng, seq, count):
    s = bytearray(seq)
    for _ in range(count):
        at = int(rng.integers(1, len(s) - 1))
        if rng.integers(0, 2):
            del s[at]
        else:
            s.insert(at, b"ACGT"[int(rng.integers(0, 4))])
    return bytes(s)


def reads_for(rng, seqs, window):
    """the edge lengths and placements for the adapters `seqs` and W = window"""
    w = window
    a = bytes(seqs[0]).upper()
    m = len(a)
    big = max(4 * w, 3 * m + 40)
    body = lambda n: random_seq(rng, max(n, 0))
    reads = [b"", b"A", b"N"]
    for n in (m - 1, m, w - 1, w, w + 1, 2 * w - 1, 2 * w, 1030):  # (1030: a read that starts on a 128-byte line)
        reads.append(body(n))
        if n >= m:
            reads.append(a + body(n - m))                          # at base 0, the read's length on an edge
            reads.append(body(n - m) + model.revcomp(a))           # at the very end
        if n >= 2 * m:
            reads.append(a + body(n - 2 * m) + model.revcomp(a))   # both ends; the two texts overlap when n < 2 W
    reads.append(a)                                                 # the adapter is the whole read: s >= e
    reads.append(a + model.revcomp(a))
    reads.append(body(3) + a + body(2))                             # nothing is left between the two cuts
    for off in (1, 5, 19):
        reads.append(body(off) + a + body(big))                     # at an offset
        reads.append(body(big) + a + body(off))
        reads.append(body(off) + model.revcomp(a) + body(big))      # in reverse complement
    if w >= m:
        reads.append(body(w - m) + a + body(big))                   # ending exactly at W
        reads.append(body(big) + a + body(w - m))
        reads.append(body(w - m + 1) + a + body(big))               # ending at W + 1: no (full) hit
        reads.append(body(big) + a + body(w - m + 1))
    for s in seqs[:3]:
        s = bytes(s).upper()
        reads.append(body(4) + substitute(rng, s, max(1, len(s) // 10)) + body(big))       # 10 % substitutions
        reads.append(body(big) + substitute(rng, s, max(1, len(s) // 10)) + body(4))
        for k in (1, 2, 3):
            reads.append(body(2) + indel(rng, s, k) + body(big))                             # 1-3-base indels
            reads.append(body(big) + indel(rng, model.revcomp(s), k) + body(2))
    reads.append(b"N" * (w + 7))                                    # N only
    reads.append(b"N" * 5 + a + b"N" * big)
    reads.append((body(3) + a + body(big)).lower())                 # lower and mixed case
    mixed = bytearray(body(3) + a + body(big) + a + body(3))
    for i in range(0, len(mixed), 2):
        mixed[i] |= 0x20
    reads.append(bytes(mixed))
    every = bytes(range(256))                                       # every byte value
    reads.append(every)
    reads.append(every[::-1] + a)
    reads.append(a[:m // 2] + every + a[m // 2:])
    reads.append(bytes(rng.integers(0, 256, size=w + 40, dtype=np.uint8)))
    reads.append(b"A" * (w + 30))                                   # a homopolymer: many j tie
    reads.append(b"A" * 9 + b"C" + b"A" * (w + 30))
    return reads


def pack(reads, fill=None):
    """plane, offsets, lengths by the plane's rule (16-byte slots, a 128-byte start from 1024 bases on).  fill: a byte string that
    is repeated through the padding and the gaps, so that a base read past a read's end is not a zero"""
    lengths = np.array([len(r) for r in reads], dtype=np.int32)
    offsets = np.zeros(max(len(reads), 1), dtype=np.uint64)
    at = 0
    for i, r in enumerate(reads):
        if len(r) >= 1024:
            at = (at + 127) & ~127
        offsets[i] = at
        at += (len(r) + 15) & ~15
    total = max(16, (at + 15) & ~15)
    if fill:
        plane = np.frombuffer((bytes(fill) * (total // len(fill) + 1))[:total], dtype=np.uint8).copy()
    else:
        plane = np.zeros(total, dtype=np.uint8)
    for r, o in zip(reads, offsets):
        if len(r):
            plane[int(o):int(o) + len(r)] = np.frombuffer(bytes(r), dtype=np.uint8)
    return plane, offsets[:len(reads)], lengths
