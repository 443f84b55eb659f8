"""The model of --exclude in numpy and Python integers (csrc/screen.h has the definition): the set X as the sorted unique uint32 codes of
both strands of the ACGT-only pieces of a contaminant, a read's hits by a rolling code and validity mask with np.isin, the decision
with Python integers.  What the kernels and the command line are held against, for equality."""
import math
from fractions import Fraction

import numpy as np

_CODE = np.full(256, 255, dtype=np.uint8)
for _i, _c in enumerate(b"ACGT"):
    _CODE[_c] = _i
    _CODE[_c + 32] = _i  # lowercase
_COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


def threshold(percent):
    """t = ceil(P / 100 * 2^32) with the quotient rounded to a double first, in exact fractions"""
    assert 0 < percent <= 100
    return math.ceil(Fraction(float(percent) / 100.0) * (1 << 32))


def pieces(seq):
    """the maximal runs of ACGTacgt of at least 16 bases, as (start, end)"""
    valid = _CODE[np.frombuffer(bytes(seq), dtype=np.uint8)] != 255
    edges = np.flatnonzero(np.diff(np.concatenate(([0], valid.view(np.uint8), [0])).astype(np.int8)))
    return [(int(a), int(b)) for a, b in zip(edges[0::2], edges[1::2]) if b - a >= 16]


def window_codes(seq):
    """(codes uint32 [windows], valid bool [windows]) of a byte string: the forward code of every 16-base window, first base on top"""
    s = np.frombuffer(bytes(seq), dtype=np.uint8)
    n = max(0, len(s) - 15)
    if n == 0:
        return np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=bool)
    c = _CODE[s]
    bad = (c == 255).astype(np.int64)
    csum = np.concatenate(([0], np.cumsum(bad)))
    valid = (csum[16:16 + n] - csum[:n]) == 0
    c2 = np.where(c == 255, 0, c).astype(np.uint64)
    codes = np.zeros(n, dtype=np.uint64)
    for k in range(16):
        codes = (codes << np.uint64(2)) | c2[k:k + n]
    return codes.astype(np.uint32), valid


def build_set(seqs):
    """X: sorted unique codes of the 16-mers of both strands of the ACGT-only pieces"""
    parts = [np.zeros(0, dtype=np.uint32)]
    for seq in seqs:
        seq = bytes(seq)
        for a, b in pieces(seq):
            piece = seq[a:b]
            parts.append(window_codes(piece)[0])
            parts.append(window_codes(piece.translate(_COMP)[::-1])[0])
    return np.unique(np.concatenate(parts))


def hits(x, read):
    codes, valid = window_codes(read)
    return int(np.count_nonzero(np.isin(codes, x) & valid))


def hits_many(x, reads):
    """hits() of every read in one pass: the rolling codes over the concatenation, every read followed by one byte outside ACGT (a
    window that reaches it is not valid, so no window belongs to two reads), then one sum per read: uint32 array"""
    n = len(reads)
    if n == 0:
        return np.zeros(0, dtype=np.uint32)
    starts = np.zeros(n, dtype=np.int64)
    starts[1:] = np.cumsum([len(r) + 1 for r in reads[:-1]])
    cat = b"\0".join(bytes(r) for r in reads) + b"\0"
    codes, valid = window_codes(cat)
    hit = np.zeros(len(cat), dtype=np.int64)  # (the last 15 bytes start no window)
    hit[:len(codes)] = np.isin(codes, x) & valid
    return np.add.reduceat(hit, starts).astype(np.uint32)  # (no segment is empty: a read of no base still has its separator)


def windows(length):
    return max(0, int(length) - 15)


def excluded(h, length, percent):
    w = windows(length)
    return w > 0 and (int(h) << 32) >= threshold(percent) * w


# ---- reads for the tests ----
def random_seq(rng, n):
    return np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=n)].tobytes()


def revcomp(seq):
    return bytes(seq).translate(_COMP)[::-1]


def mutate(rng, seq, rate):
    """substitutions at `rate`: every chosen base becomes one of the three others"""
    s = np.frombuffer(bytes(seq), dtype=np.uint8).copy()
    at = np.flatnonzero(rng.random(len(s)) < rate)
    for i in at:
        s[i] = rng.choice([c for c in b"ACGT" if c != s[i]])
    return s.tobytes()


def draw(rng, ref, length, rate=0.0, strand=None):
    """a read of `length` bases from `ref` (either strand) with substitutions at `rate`"""
    a = int(rng.integers(0, len(ref) - length + 1))
    s = ref[a:a + length]
    if strand is None:
        strand = int(rng.integers(0, 2))
    if strand:
        s = revcomp(s)
    return mutate(rng, s, rate) if rate else s
