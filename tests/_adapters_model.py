"""The model of --trim_adapters: the plain dynamic programme over the edit-distance matrix, column by column in numpy, and the keys
and children in Python integers.  Written from the definition (README), not from csrc/adapters.h: no bit vectors here.

About 1 ms per (pattern, 150-base text); patterns of one length walk a text together, which is what keeps 256 patterns affordable."""
import numpy as np

MIN_BASES, MAX_BASES, MAX_SEQS = 12, 64, 128

_CODE = np.full(256, 255, dtype=np.uint8)  # a text byte outside ACGTacgt equals no pattern base
for _i, _c in enumerate(b"ACGT"):
    _CODE[_c] = _i
    _CODE[_c + 32] = _i
_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def revcomp(seq):
    return bytes(seq).translate(_COMP)[::-1]


def patterns(seqs):
    """pattern 2 i is sequence i upper-cased, pattern 2 i + 1 its reverse complement"""
    out = []
    for s in seqs:
        s = bytes(s).upper()
        assert MIN_BASES <= len(s) <= MAX_BASES and set(s) <= set(b"ACGT"), s
        out += [s, revcomp(s)]
    assert len(out) <= 2 * MAX_SEQS
    return out


def edits_allowed(m, errors):
    return m * errors // 100


def last_rows(pats, text):
    """d(j) = D[m][j], j = 1..n, for patterns of ONE length against one text: array (len(pats), n)"""
    m, n = len(pats[0]), len(text)
    p = np.array([_CODE[np.frombuffer(q, dtype=np.uint8)] for q in pats], dtype=np.int64)  # (P, m)
    t = _CODE[np.frombuffer(bytes(text), dtype=np.uint8)].astype(np.int64)
    i = np.arange(m + 1, dtype=np.int64)
    col = np.tile(i, (len(pats), 1))  # D[.][0] = i
    out = np.zeros((len(pats), n), dtype=np.int64)
    for j in range(n):
        tmp = np.empty_like(col)
        tmp[:, 0] = 0  # D[0][j] = 0
        tmp[:, 1:] = np.minimum(col[:, :-1] + (p != t[j]), col[:, 1:] + 1)
        col = np.minimum.accumulate(tmp - i, axis=1) + i  # the vertical minimum: D[i][j] = min over i' <= i of tmp[i'] + (i - i')
        out[:, j] = col[:, m]
    return out


def end_key(read, side, window, pats, errors):
    """the key of one read end: side 0 the head, 1 the tail (the reversed read against the reversed patterns)"""
    read = bytes(read)
    n = min(len(read), window)
    if n == 0:
        return 0
    text = read[::-1][:n] if side else read[:n]
    key = 0
    by_len = {}
    for idx, q in enumerate(pats):
        by_len.setdefault(len(q), []).append(idx)
    for m, idxs in by_len.items():
        d = last_rows([pats[i][::-1] if side else pats[i] for i in idxs], text)
        for row, idx in zip(d, idxs):
            dmin = int(row.min())
            if dmin <= edits_allowed(m, errors):
                jbest = int(np.nonzero(row == dmin)[0][-1]) + 1  # the LARGEST j
                key = max(key, (jbest << 8) | idx)
    return key


def keys_of(reads, window, pats, errors):
    return np.array([[end_key(r, 0, window, pats, errors), end_key(r, 1, window, pats, errors)] for r in reads], dtype=np.uint32).reshape(-1, 2)


def child_of(length, key_head, key_tail):
    """(children, first, last): children is [] or [(s, e)]"""
    if key_head == 0 and key_tail == 0:
        return [], 0, length
    s, e = int(key_head) >> 8, length - (int(key_tail) >> 8)
    if s < e:
        return [(s, e)], s, e
    return [], -1, -1
