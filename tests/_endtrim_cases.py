"""Quality strings for the tests of --trim_ends_q, shared by the host program's tests and the GPU tests.  Every generator is seeded; the
thresholds are the library's own integers: T90 = floor(0.1 * 2^32) (the t of Q = 90), T_PLUS = E['+'] (a '+' weighs exactly zero) and
T_MID = (E['!'] + E['I']) / 2 (a '!' and an 'I' weigh +d and -d: sums come back to an earlier maximum EXACTLY)."""
import numpy as np

T90 = 429496729
T_PLUS = 429496730            # E[43]: the table entry of '+'
E_BANG, E_I = 4294967295, 429497
T_MID = (E_BANG + E_I) // 2   # 2147698396: w('!') = +2147268899 = -w('I')
assert (E_BANG + E_I) % 2 == 0


def rand_bytes(rng, n, lo, hi):
    return rng.integers(lo, hi + 1, size=n, dtype=np.uint8).tobytes()


def ont_like(rng, n, head=None, tail=None):
    """junk at both ends ('!'..'*'), a good middle ('0'..'I') with a sprinkle of bad bases"""
    head = int(rng.integers(0, 40)) if head is None else head
    tail = int(rng.integers(0, 40)) if tail is None else tail
    head, tail = min(head, n), min(tail, max(n - head, 0))
    mid = bytearray(rand_bytes(rng, n - head - tail, ord("0"), ord("I")))
    for k in rng.integers(0, max(len(mid), 1), size=len(mid) // 50):
        mid[int(k)] = int(rng.integers(33, 40))
    return rand_bytes(rng, head, 33, 42) + bytes(mid) + rand_bytes(rng, tail, 33, 42)


def edge_lengths(span):
    return [0, 1, 2, 15, 16, 17, span - 1, span, span + 1, 2 * span + 1]


def edge_reads(rng, span):
    """every edge length twice: ONT-like, and uniformly random printable bytes (cuts anywhere)"""
    out = []
    for n in edge_lengths(span):
        out.append(ont_like(rng, n))
        out.append(rand_bytes(rng, n, 33, 126))
    return out


def flat_reads(rng, span):
    """stretches of weight zero under T_PLUS: all '+', junk then '+' then good, '+' between two equal rises"""
    return [b"+" * 40, b"+", b"!!!" + b"+++++" + b"I" * 10, b"I" * 10 + b"+++++" + b"!!!",
            b"!!!" + b"+" * 100 + b"!!!" + b"I" * 50, b"+" * 7 + b"!" + b"+" * 9 + b"I" * 20,
            b"".join(rng.choice([b"+", b"+", b"!", b"I"]) for _ in range(300))]


def five_spans(span, where, side):
    """5 spans + 5 bases; the head (side 0) or tail (side 1) maximum in span `where`: junk from that end up to the middle of the span,
    with good patches inside the junk that do not outweigh it, then good quality to the other end"""
    n = 5 * span + 5
    reach = (where * span + span // 2 + 3) if side == 0 else (n - (where * span + span // 2 + 3))
    q = bytearray(b"I" * n)
    q[:reach] = b"#" * reach
    for k in range(100, reach - 100, 997):  # good patches of 20 bases: the running sum dips and recovers
        q[k:k + 20] = b"I" * 20
    return bytes(q) if side == 0 else bytes(q[::-1])


def middle_junk(longer):
    """a good flank of 200 bases ('5', Q20: w = 0.01 - 0.1 under T90), a junk stretch ('!', w = 0.9), good again: 30 junk bases outweigh
    the flank (200 * 0.09 = 18 < 27), 10 do not (9 < 18)"""
    return b"5" * 200 + b"!" * (30 if longer else 10) + b"5" * 300


def span_edge_ties(span):
    """under T_MID: the maximum of span 0 met again, exactly, behind the span's edge — the earlier one must win (and the mirror image
    for the tail); under T_PLUS: a flat stretch that straddles the edge"""
    a = b"!!!" + b"I!" * (span // 2 + 5) + b"I" * 7          # P = 3d at j = 3 and again behind every pair, in span 0 and in span 1: h = 3
    b_ = b"!" * (span - 1) + b"I!" + b"I" * 40               # the maximum at j = span - 1, met again at span + 1: h = span - 1
    c_ = b"!" * span + b"I!" + b"I" * 5                      # ... at j = span exactly, met again at span + 2: h = span
    return [(a, T_MID), (b_, T_MID), (c_, T_MID), (a[::-1], T_MID), (b_[::-1], T_MID), (c_[::-1], T_MID),
            (b"!!!" + b"+" * (span + 10) + b"I" * 9, T_PLUS), (b"I" * 9 + b"+" * (span + 10) + b"!!!", T_PLUS)]


def span_edge_tie_answers(span):
    """by hand: the head cut of the first three and of the seventh, the tail cut of their mirror images (the other cut: the model's)"""
    return [(0, 0, 3), (1, 0, span - 1), (2, 0, span), (3, 1, 3), (4, 1, span - 1), (5, 1, span), (6, 0, 3), (7, 1, 3)]


def any_bytes(rng):
    """bytes below '!' and above '~' (E is 2^32 - 1 for every byte that is no quality above 0)"""
    return [rng.integers(0, 256, size=n, dtype=np.uint8).tobytes() for n in (1, 17, 300, 2000)] + \
           [bytes([0, 5, 32, 33, 127, 128, 200, 255]) * 9, bytes([127]) * 50 + bytes([10]) * 3 + bytes([126]) * 60]


def mixed_batch(rng, n, longest):
    """n reads for the pipeline and geometry tests: ONT-like, wholly junk, wholly good, empty, one longer than a span"""
    out = []
    for i in range(n):
        kind = i % 8
        ln = int(rng.integers(1, longest))
        if kind == 5:
            out.append(rand_bytes(rng, ln % 300 + 1, 33, 38))      # all junk: h = c = L
        elif kind == 6:
            out.append(rand_bytes(rng, ln, ord("?"), ord("I")))    # all good: 0, 0
        elif kind == 7 and i % 16 == 7:
            out.append(b"")
        else:
            out.append(ont_like(rng, ln))
    return out
