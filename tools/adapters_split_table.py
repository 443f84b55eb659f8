#!/usr/bin/env python3
"""What the definition of --split_adapters costs and finds, computed with the models of tests/ (no GPU): the tables of README.md.
  false hits   false middle hits per Mbp of random sequence, for random patterns of m bases at E2 % edits (one pattern, one strand):
               maximal runs of hit ends, each of which would split a read; and from that the share of 10 kbp reads that a set of two
               sequences (four patterns) splits falsely
  detection    the 28-base ligation adapter with three random edits between two random 2 kbp halves: how often the read is split,
               and how far the two child edges lie from the true junction (the adapter's first and last base)"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import _adapters_cases as cases  # noqa: E402
import _adapters_model as model  # noqa: E402
import _adapters_split_model as split  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mbp", type=float, default=1.0, help="random sequence per pattern length")
    ap.add_argument("--patterns", type=int, default=4)
    ap.add_argument("--reads", type=int, default=300)
    ap.add_argument("--split_errors", type=int, default=10)
    args = ap.parse_args()
    rng = np.random.default_rng(2027)
    n = int(args.mbp * 1e6)
    for m in (12, 16, 20, 24, 28):
        pats = [cases.random_seq(rng, m) for _ in range(args.patterns)]
        d = model.last_rows(pats, cases.random_seq(rng, n))
        for e2 in (10, 20):
            hit = d <= model.edits_allowed(m, e2)
            runs = int((hit[:, 1:] & ~hit[:, :-1]).sum() + hit[:, 0].sum())
            per_mbp = runs / (args.patterns * n / 1e6)
            share = 1.0 - np.exp(-per_mbp * 4 * 0.01)  # four patterns over 10 kbp
            print("m = %2d  E2 = %2d  k2 = %d  false hits per Mbp and pattern: %8.1f   10 kbp reads split falsely by two sequences: %5.1f %%"
                  % (m, e2, model.edits_allowed(m, e2), per_mbp, 100.0 * share))
    pats = model.patterns([cases.LIGATION])
    found, left, right = 0, [], []
    for _ in range(args.reads):
        s = bytearray(cases.LIGATION)
        for _e in range(3):
            at, kind = int(rng.integers(0, len(s))), int(rng.integers(0, 3))
            if kind == 0:
                s[at] = b"ACGT"[(b"ACGT".index(s[at]) + int(rng.integers(1, 4))) % 4]
            elif kind == 1:
                s.insert(at, b"ACGT"[int(rng.integers(0, 4))])
            else:
                del s[at]
        read = cases.random_seq(rng, 2000) + bytes(s) + cases.random_seq(rng, 2000)
        ch = split.children(len(read), 0, 0, split.marks(read, pats, args.split_errors))[0]
        if len(ch) == 2:
            found += 1
            left.append(ch[0][1] - 2000)
            right.append(ch[1][0] - (2000 + len(s)))
    for name, v in (("first child's end minus the adapter's first base", left), ("second child's start minus the adapter's end", right)):
        values, counts = np.unique(v, return_counts=True)
        print("%s: %s" % (name, dict(zip(values.tolist(), counts.tolist()))))
    print("ligation adapter, 3 edits, E2 = %d: split in two in %d of %d reads" % (args.split_errors, found, args.reads))


if __name__ == "__main__":
    main()
