"""The model of --adapter_overhang: both walks of a (text, pattern) pair as the plain dynamic programme over the edit-distance matrix,
column by column in numpy, and the key rule in Python integers.  Written from the definition (README), not from
csrc/adapters.h: no bit vectors here.

  free walk      D[0][j] = 0, D[i][0] = i: the whole pattern anywhere in the text, k = m * E / 100 edits
  anchored walk  D[0][j] = j, D[i][0] = max(0, i - O_p): the occurrence begins at the text's first base and the first O_p pattern
                 bases may be missing; O_p = min(O, m - 12), k' = (m - O_p) * E / 100 edits; only where O_p > 0
  key            max over every hitting walk of every pattern of (jbest << 8) | pattern, jbest the largest j with the walk's minimum

Patterns of one length walk every text of a batch together (about 0.2 s per pattern length, walk and 150-base window, however many
texts); patterns(), revcomp() and child_of() of tests/_adapters_model.py serve here too."""
import numpy as np

from _adapters_model import MIN_BASES, MAX_BASES, child_of, patterns, revcomp  # noqa: F401 (handed on to the tests)

MAX_OVERHANG = MAX_BASES - MIN_BASES

_CODE = np.full(256, 255, dtype=np.uint8)  # a text byte outside ACGTacgt equals no pattern base
for _i, _c in enumerate(b"ACGT"):
    _CODE[_c] = _i
    _CODE[_c + 32] = _i


def overhang_of(m, overhang):
    """O_p"""
    return min(overhang, m - MIN_BASES)


def edits_allowed(m, errors):
    """k of the free walk"""
    return m * errors // 100


def edits_anchored(m, errors, overhang):
    """k'_p"""
    return (m - overhang_of(m, overhang)) * errors // 100


def last_rows_many(pats, texts, free_rows=None):
    """d(j) = D[m][j], j = 1..len(text), for patterns of ONE length against many texts at once: array (len(texts), len(pats), longest
    text); what lies behind a text's own length means nothing.  free_rows None: the free walk; an integer o: the anchored walk whose
    first o pattern bases may be missing"""
    m, n = len(pats[0]), max(len(t) for t in texts)
    p = np.array([_CODE[np.frombuffer(q, dtype=np.uint8)] for q in pats], dtype=np.int32)  # (P, m)
    t = np.full((len(texts), n), 254, dtype=np.int32)  # (T, n), padded with a code that equals nothing
    for k, text in enumerate(texts):
        t[k, :len(text)] = _CODE[np.frombuffer(bytes(text), dtype=np.uint8)]
    i = np.arange(m + 1, dtype=np.int32)
    first = i if free_rows is None else np.maximum(0, i - free_rows)  # D[.][0]
    col = np.broadcast_to(first, (len(texts), len(pats), m + 1)).copy()
    out = np.zeros((len(texts), len(pats), n), dtype=np.int32)
    for j in range(n):
        tmp = np.empty_like(col)
        tmp[:, :, 0] = 0 if free_rows is None else j + 1  # D[0][j]
        tmp[:, :, 1:] = np.minimum(col[:, :, :-1] + (p[None, :, :] != t[:, j, None, None]), col[:, :, 1:] + 1)
        col = np.minimum.accumulate(tmp - i, axis=2) + i  # the vertical minimum: D[i][j] = min over i' <= i of tmp[i'] + (i - i')
        out[:, :, j] = col[:, :, m]
    return out


def last_rows(pats, text, free_rows=None):
    """the same for one text: array (len(pats), len(text))"""
    return last_rows_many(pats, [text], free_rows)[0]


def walk(row, allowed):
    """(dmin, jbest) of a walk that hits, None of one that does not"""
    dmin = int(row.min())
    if dmin > allowed:
        return None
    return dmin, int(np.nonzero(row == dmin)[0][-1]) + 1  # the LARGEST j


def walks_of_texts(texts, side, pats, errors, overhang):
    """for every text (a head text as it stands in the read; a tail text already REVERSED, side 1: against the reversed patterns)
    the list, per pattern, of (free, anchored): each None or (dmin, jbest)"""
    out = [[(None, None)] * len(pats) for _ in texts]
    live = [k for k, t in enumerate(texts) if len(t)]
    if not live:
        return out
    by_len = {}
    for idx, q in enumerate(pats):
        by_len.setdefault(len(q), []).append(idx)
    for m, idxs in by_len.items():
        qs = [pats[i][::-1] if side else pats[i] for i in idxs]
        o = overhang_of(m, overhang)
        free = last_rows_many(qs, [texts[k] for k in live])
        anchored = last_rows_many(qs, [texts[k] for k in live], o) if o > 0 else None
        for at, k in enumerate(live):
            n = len(texts[k])
            for col, idx in enumerate(idxs):
                out[k][idx] = (walk(free[at, col, :n], edits_allowed(m, errors)),
                               None if anchored is None else walk(anchored[at, col, :n], edits_anchored(m, errors, overhang)))
    return out


def text_of(read, side, window):
    read = bytes(read)
    n = min(len(read), window)
    return read[::-1][:n] if side else read[:n]


def end_walks(read, side, window, pats, errors, overhang):
    """per pattern (free, anchored) of one read end: side 0 the head, 1 the tail (the reversed read against the reversed patterns)"""
    return walks_of_texts([text_of(read, side, window)], side, pats, errors, overhang)[0]


def key_of_walks(walks, anchored=True):
    """anchored False: of the free walks alone, which is the key at O = 0"""
    key = 0
    for idx, both in enumerate(walks):
        for w in both if anchored else both[:1]:
            if w is not None:
                key = max(key, (w[1] << 8) | idx)
    return key


def end_key(read, side, window, pats, errors, overhang):
    return key_of_walks(end_walks(read, side, window, pats, errors, overhang))


def keys_of(reads, window, pats, errors, overhang, cache=None, with_plain=False):
    """[n, 2] keys.  An end's key depends on the W bases at that end alone: every DISTINCT text is walked once, all of them together.
    cache: {(side, text): (key, key at O = 0)}, kept by a caller that asks about the same texts again.  with_plain: (keys, the keys
    of the free walks alone), from the same walks"""
    cache = {} if cache is None else cache
    texts = [[text_of(r, side, window) for r in reads] for side in (0, 1)]
    for side in (0, 1):
        new = sorted({t for t in texts[side] if (side, t) not in cache})
        for t, walks in zip(new, walks_of_texts(new, side, pats, errors, overhang)):
            cache[(side, t)] = (key_of_walks(walks), key_of_walks(walks, anchored=False))
    both = [np.array([[cache[(0, h)][k], cache[(1, t)][k]] for h, t in zip(texts[0], texts[1])], dtype=np.uint32).reshape(-1, 2) for k in (0, 1)]
    return (both[0], both[1]) if with_plain else both[0]
