"""The model of --max_low_complexity in numpy and Python integers (csrc/complexity.h has the definition): per window the triplet
histogram from scratch (64 prefix sums of the triplet kinds, one difference per window and kind — no sliding score), then S, validity,
bad, windows and the decision through api.screen_threshold.  What the host walk, the kernel and the command line are held against,
for equality.  Also the generators of the tests and of tools/complexity_table.py."""
import numpy as np

WINDOW = 64
TRIPLETS = WINDOW - 2

_CODE = np.full(256, 255, dtype=np.uint8)
for _i, _c in enumerate(b"ACGT"):
    _CODE[_c] = _i
    _CODE[_c + 32] = _i  # lowercase


def windows(length):
    return max(0, int(length) - (WINDOW - 1))


def window_scores(seq):
    """(S int64 [windows], valid bool [windows]) of a byte string: for every window start the pairs of equal triplets among the
    window's 62 triplets, and whether its 64 bytes are all in ACGTacgt (S of a window that is not valid means nothing)"""
    s = np.frombuffer(bytes(seq), dtype=np.uint8)
    n = windows(len(s))
    if n == 0:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=bool)
    c = _CODE[s]
    inv = np.concatenate(([0], np.cumsum(c == 255)))
    valid = (inv[WINDOW:WINDOW + n] - inv[:n]) == 0
    c = np.where(c == 255, 0, c).astype(np.int64)
    kinds = c[:-2] * 16 + c[1:-1] * 4 + c[2:]  # the triplet that starts at every base
    S = np.zeros(n, dtype=np.int64)
    for t in range(64):
        cs = np.concatenate(([0], np.cumsum(kinds == t)))
        ct = cs[TRIPLETS:TRIPLETS + n] - cs[:n]
        S += ct * (ct - 1) // 2
    return S, valid


def is_bad(S, T):
    return 10 * S > int(T) * (WINDOW - 3)


def bad_windows(seq, T=20):
    S, valid = window_scores(seq)
    return int(np.count_nonzero(valid & is_bad(S, T)))


def bad_many(reads, T=20):
    """bad_windows() of every read in one pass: the scores over the concatenation, every read followed by one byte outside ACGT (a
    window that reaches it is not valid, so no window belongs to two reads), then one sum per read: uint32 array"""
    n = len(reads)
    if n == 0:
        return np.zeros(0, dtype=np.uint32)
    starts = np.zeros(n, dtype=np.int64)
    starts[1:] = np.cumsum([len(r) + 1 for r in reads[:-1]])
    cat = b"\0".join(bytes(r) for r in reads) + b"\0"
    S, valid = window_scores(cat)
    hit = np.zeros(len(cat), dtype=np.int64)  # (the last 63 bytes start no window)
    hit[:len(S)] = valid & is_bad(S, T)
    return np.add.reduceat(hit, starts).astype(np.uint32)  # (no segment is empty: a read of no base still has its separator)


def flagged(bad, length, percent):
    from filtlong_amd import api
    w = windows(length)
    return w > 0 and (int(bad) << 32) >= api.screen_threshold(percent) * w


def flagged_many(bad, lengths, percent):
    return np.array([flagged(b, n, percent) for b, n in zip(bad, lengths)], dtype=np.uint8)


# ---- generators ----
_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def random_seq(rng, n, gc=0.5):
    p = [(1 - gc) / 2, gc / 2, gc / 2, (1 - gc) / 2]
    return _ACGT[rng.choice(4, size=n, p=p)].tobytes()


def mutate(rng, seq, rate):
    """substitutions at `rate`: every chosen base becomes one of the three others"""
    s = np.frombuffer(bytes(seq), dtype=np.uint8).copy()
    at = np.flatnonzero(rng.random(len(s)) < rate)
    if len(at):
        cur = _CODE[s[at]].astype(np.int64)
        s[at] = _ACGT[(cur + rng.integers(1, 4, size=len(at))) % 4]
    return s.tobytes()


def repeat(rng, period, n, rate=0.0):
    """n bases of an exact repeat of a random unit of `period` bases that is no repeat of a shorter unit, then substitutions"""
    while True:
        unit = random_seq(rng, period)
        if all(unit != unit[:d] * (period // d) for d in range(1, period) if period % d == 0):
            break
    s = (unit * (n // period + 1))[:n]
    return mutate(rng, s, rate) if rate else s


def _score64(codes):
    k = codes[:-2] * 16 + codes[1:-1] * 4 + codes[2:]
    c = np.bincount(k, minlength=64)
    return int((c * (c - 1) // 2).sum())


def window_with_score(rng, target, tries=30000):
    """64 bases of ACGT whose S is exactly `target`, by a local search from a homopolymer or a random window; None if it finds none
    (some values have no window: 1831 is not a sum of c (c - 1) / 2 over counts that add up to 62)"""
    codes = np.zeros(WINDOW, dtype=np.int64) if target > 900 else rng.integers(0, 4, size=WINDOW)
    cur = _score64(codes)
    for _ in range(tries):
        if cur == target:
            return _ACGT[codes].tobytes()
        i, v = int(rng.integers(0, WINDOW)), int(rng.integers(0, 4))
        old = int(codes[i])
        if v == old:
            continue
        codes[i] = v
        new = _score64(codes)
        if abs(new - target) <= abs(cur - target):
            cur = new
        else:
            codes[i] = old
    return None


def borderline(rng, T):
    """(a window with S = floor(T * 61 / 10): good, a window with one more: bad) — either may be None"""
    edge = int(T) * (WINDOW - 3) // 10
    return window_with_score(rng, edge), window_with_score(rng, edge + 1)
