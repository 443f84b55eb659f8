#!/usr/bin/env python3
"""What --adapter_overhang O finds and what it finds falsely, computed with the model of tests/_adapters_overhang_model.py (no GPU):
the table of README.md.
  detection    the 28-base ligation adapter truncated by x = 0, 2, ..., 16 bases at the read's first base, three random edits in what
               is left, in front of random sequence: in how many of --reads reads the head is cut, at O = 0, 4, 8, 12, 16 (E % edits)
  false hits   per 1000 random windows of W bases, for random patterns of m = 12, 16, 20, 28, 40 bases at the same O (one pattern, one
               strand, one end; O = 0 is the free walk alone, the others count the windows either walk hits)"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import _adapters_cases as cases  # noqa: E402
import _adapters_overhang_model as model  # noqa: E402

OVERHANGS = (0, 4, 8, 12, 16)


def edited(rng, seq, edits):
    s = bytearray(seq)
    for _ in range(edits):
        at, kind = int(rng.integers(0, len(s))), int(rng.integers(0, 3))
        if kind == 0:
            s[at] = b"ACGT"[(b"ACGT".index(s[at]) + int(rng.integers(1, 4))) % 4]
        elif kind == 1:
            s.insert(at, b"ACGT"[int(rng.integers(0, 4))])
        elif len(s) > 1:
            del s[at]
    return bytes(s)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=int, default=150)
    ap.add_argument("--errors", type=int, default=20)
    ap.add_argument("--patterns", type=int, default=5)
    ap.add_argument("--windows", type=int, default=1000)
    ap.add_argument("--reads", type=int, default=300)
    args = ap.parse_args()
    rng = np.random.default_rng(2027)
    a = cases.LIGATION
    print("ligation adapter (28 bases) truncated by x, 3 edits in the rest, E = %d: reads of %d whose head is cut" % (args.errors, args.reads))
    print("  x  " + "".join("  O = %-3d" % o for o in OVERHANGS))
    for x in range(0, 17, 2):
        texts = [edited(rng, a[x:], 3) + cases.random_seq(rng, args.window) for _ in range(args.reads)]
        row = [int((model.keys_of(texts, args.window, [a], args.errors, o)[:, 0] > 0).sum()) for o in OVERHANGS]
        print(" %2d  " % x + "".join("  %-7d" % v for v in row))
    print("false hits per 1000 random %d-base windows, random patterns of m bases, E = %d (k' in brackets)" % (args.window, args.errors))
    print("  m  " + "".join("  O = %-7d" % o for o in OVERHANGS))
    for m in (12, 16, 20, 28, 40):
        pats = [cases.random_seq(rng, m) for _ in range(args.patterns)]
        texts = [cases.random_seq(rng, args.window) for _ in range(args.windows)]
        row = []
        for o in OVERHANGS:
            hits = sum(int((model.keys_of(texts, args.window, [p], args.errors, o)[:, 0] > 0).sum()) for p in pats)
            row.append("%.1f (%d)" % (1000.0 * hits / (args.patterns * args.windows), model.edits_anchored(m, args.errors, o)))
        print(" %2d  " % m + "".join("  %-11s" % v for v in row))


if __name__ == "__main__":
    main()
