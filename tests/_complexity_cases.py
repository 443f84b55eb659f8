"""Reads for the tests of --max_low_complexity: the edge cases the host program and the kernel share, and the mixed batch."""
import numpy as np

import _complexity_model as model


def edge_reads(rng, span):
    """lengths around the window and the span, lower case, single N bytes, all N, homopolymers, as a list of byte strings"""
    reads = []
    for n in (0, 1, 62, 63, 64, 65, 126, 127, 128, span + 62, span + 63, span + 64):
        reads.append(model.repeat(rng, 3, n))                      # every window bad
        reads.append(model.random_seq(rng, n))                     # (nearly) no window bad
        reads.append(model.repeat(rng, 2, n).lower())
        half = model.repeat(rng, 1, n // 2) + model.random_seq(rng, n - n // 2)
        reads.append(half)
        for at in (0, 62, 63, 64, n - 1):
            if 0 <= at < n:
                s = bytearray(model.repeat(rng, 2, n))
                s[at] = ord("N")
                reads.append(bytes(s))
    reads.append(b"N" * 300)
    reads.append(b"A" * 64)   # one window, and it is bad
    reads.append(b"A" * 63)   # no window
    reads.append(b"acgt" * 40)
    return reads


def borderline_reads(rng, T):
    """the two windows of the model's search at T (those that exist), alone and inside random sequence"""
    out = []
    for w in model.borderline(rng, T):
        if w is not None:
            out.append(w)
            out.append(model.random_seq(rng, 70) + w + model.random_seq(rng, 70))
    return out


def mixed_batch(rng, n=200):
    """about n reads of 64..6000 bases: random reads, repeats of period 1..12, half repeat and half random, repeat islands of 40,
    64, 65 and 200 bases, N runs"""
    reads = []
    for i in range(n):
        L = int(rng.integers(64, 6001))
        kind = i % 5
        if kind == 0:
            r = model.random_seq(rng, L, gc=float(rng.choice([0.2, 0.5, 0.8])))
        elif kind == 1:
            r = model.repeat(rng, 1 + i // 5 % 12, L, rate=float(rng.choice([0.0, 0.05, 0.1])))
        elif kind == 2:
            r = model.repeat(rng, 1 + i // 5 % 12, L // 2) + model.random_seq(rng, L - L // 2)
        elif kind == 3:
            s = bytearray(model.random_seq(rng, L))
            for isl in (40, 64, 65, 200):
                if L > isl + 2:
                    a = int(rng.integers(0, L - isl))
                    s[a:a + isl] = model.repeat(rng, int(rng.integers(1, 4)), isl)
            r = bytes(s)
        else:
            s = bytearray(model.repeat(rng, 1 + i // 5 % 6, L))
            for _ in range(3):
                a, m = int(rng.integers(0, L)), int(rng.integers(1, 80))
                s[a:a + m] = b"N" * len(s[a:a + m])
            r = bytes(s)
        reads.append(r)
    return reads


def straddle(rng, length, edge, island, period=2):
    """a random read of `length` bases with a repeat island of `island` bases whose middle sits on base `edge`"""
    s = bytearray(model.random_seq(rng, length))
    a = max(0, min(length - island, edge - island // 2))
    if length >= island:
        s[a:a + island] = model.repeat(rng, period, island)
    return bytes(s)
