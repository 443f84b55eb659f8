#!/usr/bin/env python3
"""What the definition of --trim_adapters costs and finds, computed with the model of tests/_adapters_model.py (no GPU): the table of
README.md.
  false hits   per 1000 random windows of W bases, for random patterns of m bases at E % edits (one pattern, one strand, one end)
  detection    the 28-base ligation adapter with three random edits (10 %) behind 0 to 19 random bases: how often it is found and where
               the cut lands relative to the true end of the adapter"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import _adapters_cases as cases  # noqa: E402
import _adapters_model as model  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=int, default=150)
    ap.add_argument("--errors", type=int, default=20)
    ap.add_argument("--patterns", type=int, default=5)
    ap.add_argument("--windows", type=int, default=1000)
    ap.add_argument("--reads", type=int, default=300)
    args = ap.parse_args()
    rng = np.random.default_rng(2026)
    for m in (8, 12, 16, 20, 24, 28):
        hits = 0
        for _ in range(args.patterns):
            pat = cases.random_seq(rng, m)
            for _ in range(args.windows):
                d = model.last_rows([pat], cases.random_seq(rng, args.window))[0]
                hits += int(d.min()) <= model.edits_allowed(m, args.errors)
        print("m = %2d  k = %d  false hits per 1000 windows: %.1f" % (m, model.edits_allowed(m, args.errors), 1000.0 * hits / (args.patterns * args.windows)))
    found, where = 0, []
    for _ in range(args.reads):
        lead = int(rng.integers(0, 20))
        s = bytearray(cases.LIGATION)
        for _e in range(3):
            at, kind = int(rng.integers(0, len(s))), int(rng.integers(0, 3))
            if kind == 0:
                s[at] = b"ACGT"[(b"ACGT".index(s[at]) + int(rng.integers(1, 4))) % 4]
            elif kind == 1:
                s.insert(at, b"ACGT"[int(rng.integers(0, 4))])
            else:
                del s[at]
        read = cases.random_seq(rng, lead) + bytes(s) + cases.random_seq(rng, 400)
        key = model.end_key(read, 0, args.window, [cases.LIGATION], args.errors)
        if key:
            found += 1
            where.append((key >> 8) - (lead + len(s)))
    values, counts = np.unique(where, return_counts=True)
    print("ligation adapter, 3 edits: found in %d of %d reads; cut minus true end: %s" % (found, args.reads, dict(zip(values.tolist(), counts.tolist()))))


if __name__ == "__main__":
    main()
