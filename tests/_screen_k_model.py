"""The model of --exclude_k in numpy and Python integers (csrc/screen_hash.h has the definition): tests/_screen_model.py with 16
replaced by K, 16 <= K <= 31.  uint64 rolling codes, the canonical key as the smaller of a window's code and its reverse complement's,
X as the sorted unique canonical keys of the reference, a read's hits with np.isin, the decision with Python integers.  What the
kernels and the command line are held against, for equality."""
import numpy as np

import _screen_model as base
from _screen_model import draw, mutate, random_seq, revcomp, threshold  # noqa: F401  (the tests take them from here)

_CODE = base._CODE


def windows(length, k):
    return max(0, int(length) - k + 1)


def window_keys(seq, k):
    """(canonical keys uint64 [windows], valid bool [windows]) of a byte string: every window of k bases"""
    s = np.frombuffer(bytes(seq), dtype=np.uint8)
    n = windows(len(s), k)
    if n == 0:
        return np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=bool)
    c = _CODE[s]
    bad = (c == 255).astype(np.int64)
    csum = np.concatenate(([0], np.cumsum(bad)))
    valid = (csum[k:k + n] - csum[:n]) == 0
    c2 = np.where(c == 255, 0, c).astype(np.uint64)
    fwd = np.zeros(n, dtype=np.uint64)
    rc = np.zeros(n, dtype=np.uint64)
    for i in range(k):
        fwd = (fwd << np.uint64(2)) | c2[i:i + n]
        rc = rc | ((np.uint64(3) - c2[i:i + n]) << np.uint64(2 * i))  # the complement of base i is base k - 1 - i of the other strand
    return np.minimum(fwd, rc), valid


def key_of(kmer):
    """the canonical key of one K-mer of ACGT, in Python integers"""
    code = {65: 0, 67: 1, 71: 2, 84: 3}
    fwd = rc = 0
    for i, ch in enumerate(bytes(kmer).upper()):
        fwd = (fwd << 2) | code[ch]
        rc |= (3 - code[ch]) << (2 * i)
    return min(fwd, rc)


def build_set(seqs, k):
    """X_K: the sorted unique canonical keys of the valid windows of every sequence (a window's key is its reverse complement's)"""
    parts = [np.zeros(0, dtype=np.uint64)]
    for seq in seqs:
        keys, valid = window_keys(seq, k)
        parts.append(keys[valid])
    return np.unique(np.concatenate(parts))


def hits(x, read, k):
    keys, valid = window_keys(read, k)
    return int(np.count_nonzero(np.isin(keys, x) & valid))


def hits_many(x, reads, k):
    """hits() of every read in one pass: the rolling keys over the concatenation, every read followed by one byte outside ACGT (a
    window that reaches it is not valid, so no window belongs to two reads), then one sum per read: uint32 array"""
    n = len(reads)
    if n == 0:
        return np.zeros(0, dtype=np.uint32)
    starts = np.zeros(n, dtype=np.int64)
    starts[1:] = np.cumsum([len(r) + 1 for r in reads[:-1]])
    cat = b"\0".join(bytes(r) for r in reads) + b"\0"
    keys, valid = window_keys(cat, k)
    hit = np.zeros(len(cat), dtype=np.int64)  # (the last k - 1 bytes start no window)
    hit[:len(keys)] = np.isin(keys, x) & valid
    return np.add.reduceat(hit, starts).astype(np.uint32)  # (no segment is empty: a read of no base still has its separator)


def excluded(h, length, percent, k):
    w = windows(length, k)
    return w > 0 and (int(h) << 32) >= threshold(percent) * w
