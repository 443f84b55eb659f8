"""The model of --split_adapters: the plain dynamic programme of tests/_adapters_model.py over the WHOLE read, then the marks, their
union and the children in numpy and Python integers.  Written from the definition (README), not from csrc/adapters.h:
no bit vectors, no pieces, no warm-up here.

    hit ends   d_p(j) = D[m][j] over the whole read, j = 1..L; j is a hit end of pattern p iff d_p(j) <= k2 = m * E2 // 100
    marks      every hit end (p, j) marks the bases [max(0, j - m), j); B is the union
    children   [s, e) is what the ends rule leaves.  No end hit and B empty: no child, first = 0, last = L.  Otherwise the maximal
               runs of bases of [s, e) outside B; no base left: no child, first = last = -1."""
import numpy as np

import _adapters_model as model


def marks(read, pats, split_errors):
    """B as a boolean array of L entries"""
    read = bytes(read)
    L = len(read)
    delta = np.zeros(L + 1, dtype=np.int64)  # +1 where a mark begins, -1 where it ends
    if L:
        by_len = {}
        for q in pats:
            by_len.setdefault(len(q), []).append(q)
        for m, qs in by_len.items():
            k2 = model.edits_allowed(m, split_errors)
            d = model.last_rows(qs, read)  # (patterns of this length, L): column j - 1 is d(j)
            ends = np.unique(np.nonzero(d <= k2)[1]) + 1
            np.add.at(delta, np.maximum(ends - m, 0), 1)
            np.add.at(delta, ends, -1)
    return np.cumsum(delta)[:L] > 0


def children(length, key_head, key_tail, marked):
    """(children [(s, e), ...], first, last)"""
    end_hit = key_head != 0 or key_tail != 0
    if not end_hit and not marked.any():
        return [], 0, length
    s, e = int(key_head) >> 8, length - (int(key_tail) >> 8)
    free = np.zeros(length + 2, dtype=np.int8)  # base i at i + 1, a bad base on either side
    if s < e:
        free[s + 1:e + 1] = ~marked[s:e]
    step = np.diff(free)
    starts, ends = np.nonzero(step == 1)[0], np.nonzero(step == -1)[0]
    ch = [(int(a), int(b)) for a, b in zip(starts, ends)]
    if not ch:
        return [], -1, -1
    return ch, ch[0][0], ch[-1][1]


def split_of(read, window, pats, errors, split_errors):
    """(key_head, key_tail, marks, children, first, last) of one read"""
    kh, kt = model.end_key(read, 0, window, pats, errors), model.end_key(read, 1, window, pats, errors)
    b = marks(read, pats, split_errors)
    ch, first, last = children(len(read), kh, kt, b)
    return kh, kt, b, ch, first, last
