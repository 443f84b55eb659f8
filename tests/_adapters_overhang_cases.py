"""Reads for the --adapter_overhang tests: adapters that the read begins or ends inside, at every edge the definition has, for one
(adapter set, E, W, O).  Truncation x at the head: the read begins with adapter[x:]; at the tail: the read ends with adapter[:m - x]
(the reversed pattern's first x bases, the adapter's last, are the missing ones)."""
import numpy as np

import _adapters_cases as cases
import _adapters_overhang_model as model


def head_remnant(a, x):
    return a[x:]


def tail_remnant(a, x):
    return a[:len(a) - x]


def with_n_and_lower(remnant):
    """an N at a third of the remnant, lower case from its middle on"""
    r = bytearray(remnant)
    r[len(r) // 3] = ord("N")
    r[len(r) // 2:] = bytes(r[len(r) // 2:]).lower()
    return bytes(r)


def reads_for(rng, seqs, errors, window, overhang, planted=3):
    """the edge lengths and truncations for the first `planted` adapters of `seqs`"""
    w = window
    big = max(2 * w + 40, 200)
    body = lambda n: cases.random_seq(rng, max(n, 0))
    reads = [b"", b"A", b"N", body(w), body(big)]
    for s in seqs[:planted]:
        a = bytes(s).upper()
        m = len(a)
        o, k = model.overhang_of(m, overhang), model.edits_anchored(m, errors, overhang)
        # the lengths: the remnant cut to L bases at the head, the last L bases of a read that ends in the remnant
        for n in sorted({0, 1, m - o - 1, m - o, m - o + k, m + k, m + k + 1, w - 1, w, w + 1}):
            if n < 0:
                continue
            reads.append((head_remnant(a, o) + body(big))[:n])
            ends = body(big) + tail_remnant(a, o)
            reads.append(ends[len(ends) - n:])
        for both in (a, model.revcomp(a)):
            # the truncations around O_p, and the first one the allowance cannot pay for
            for x in sorted({max(o - 1, 0), o, min(o + 1, m - 1), min(o + k + 1, m - 1), o // 2}):
                reads.append(head_remnant(both, x) + body(big))
                reads.append(body(big) + tail_remnant(both, x))
                reads.append(head_remnant(both, x) + body(big) + tail_remnant(model.revcomp(both), x))  # both ends of one read
        for x in sorted({o, max(o - 1, 0), o // 2}):
            rem = head_remnant(a, x)
            for e in sorted({0, 1, k, k + 1}):  # edits inside the remnant, up to one more than the allowance
                if e <= len(rem) - 2:
                    reads.append(cases.substitute(rng, rem, e) + body(big))
                    reads.append(body(big) + cases.substitute(rng, tail_remnant(a, x), e))
            if len(rem) > 6:
                reads.append(cases.indel(rng, rem, 1) + body(big))
                reads.append(body(big) + cases.indel(rng, tail_remnant(a, x), 2))
            reads.append(with_n_and_lower(rem) + body(big))                     # an N and lower case inside the remnant
            reads.append(body(big) + with_n_and_lower(tail_remnant(a, x)))
            reads.append((rem + body(big)).lower())
        # both walks hit, at different j: the remnant at the edge and the whole adapter a few bases behind it
        reads.append(head_remnant(a, o) + body(3) + a + body(big))
        reads.append(body(big) + model.revcomp(a) + body(2) + tail_remnant(model.revcomp(a), o))
        reads.append(head_remnant(a, max(o, 1)))                                  # the remnant is the whole read
        reads.append(a)
        reads.append(body(2) + head_remnant(a, o) + body(big))                    # a remnant NOT at the edge: two edits of the anchored walk
    reads.append(b"N" * (w + 3))
    reads.append(b"A" * (w + 30))  # a homopolymer: many j tie
    reads.append(bytes(range(256)))
    return reads
