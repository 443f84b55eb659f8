"""--trim_ends_q restated in plain Python and numpy, for the tests: integer prefix sums of w(b) = E[b] - t over the table of
--split_window_q (api.qsplit_table(): the library hands it over without a device), the head cut at the SMALLEST j at
which P(j) is maximal, the tail cut at the smallest c at which S(c) is maximal, and the child rule of the adapter ends.  Everything is
int64 (|w| < 2^32 and L < 2^31) and no float is involved."""
import numpy as np

_TABLE = None


def table():
    """E[0..255], uint32 (csrc/qsplit.h)"""
    global _TABLE
    if _TABLE is None:
        from filtlong_amd import api
        _TABLE = api.qsplit_table().astype(np.int64)
    return _TABLE


def weights(qual, t):
    q = np.frombuffer(bytes(qual), dtype=np.uint8)
    return table()[q] - np.int64(t)


def cuts(qual, t):
    """(h, c) of one quality string"""
    if len(qual) == 0:
        return 0, 0
    w = weights(qual, t)
    P = np.concatenate(([0], np.cumsum(w)))          # P[j], 0 <= j <= L
    S = np.concatenate(([0], np.cumsum(w[::-1])))    # S[c], 0 <= c <= L
    return int(np.argmax(P)), int(np.argmax(S))      # (argmax: the first, i.e. the smallest, index of the maximum)


def cuts_walk(qual, t):
    """the same by the serial walk, in Python integers: what cuts() is checked against"""
    E = table()
    h = c = 0
    run = best = 0
    for j, b in enumerate(bytes(qual)):
        run += int(E[b]) - int(t)
        if run > best:
            best, h = run, j + 1
    run = best = 0
    for k, b in enumerate(bytes(qual)[::-1]):
        run += int(E[b]) - int(t)
        if run > best:
            best, c = run, k + 1
    return h, c


def child_of(h, c, L):
    """(children, first, last) by the rule of the adapter ends"""
    if h == 0 and c == 0:
        return 0, 0, L
    s, e = h, L - c
    if s < e:
        return 1, s, e
    return 0, -1, -1


def batch_cuts(quals, t):
    return np.array([cuts(q, t) for q in quals], dtype=np.uint32).reshape(-1, 2)
