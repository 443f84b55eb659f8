#!/usr/bin/env python3
"""What --max_low_complexity catches and what it leaves, from the model of the tests (tests/_complexity_model.py; no GPU): the share
of bad 64-base windows, in percent, at --low_complexity_score T = 10, 20 and 30
  random    for 200 kbp of random sequence at several GC contents, with the mean and the largest window score S
  period p  for exact repeats of p = 1 .. 20 bases (16 random units that are no repeat of a shorter one, 4 kbp each, pooled), with
            0, 5 and 10 % substitutions
printed as the Markdown tables of README.md."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import _complexity_model as model  # noqa: E402

SCORES = (10, 20, 30)


def shares(seqs):
    """(S of all windows of the sequences, the share of bad windows at every T as text)"""
    scored = [model.window_scores(s) for s in seqs]
    S, valid = np.concatenate([a for a, _ in scored]), np.concatenate([b for _, b in scored])
    return S, ["%.1f" % (100.0 * np.count_nonzero(valid & model.is_bad(S, T)) / len(S)) for T in SCORES]


def main():
    rng = np.random.default_rng(2025)
    print("| random sequence, GC | mean S | max S | " + " | ".join("bad at T = %d" % T for T in SCORES) + " |")
    print("|---|---|---|" + "---|" * len(SCORES))
    for gc in (0.5, 0.4, 0.3, 0.2, 0.1):
        S, row = shares([model.random_seq(rng, 200000, gc=gc)])
        print("| %d %% | %.1f | %d | " % (round(100 * gc), S.mean(), S.max()) + " | ".join(r + " %" for r in row) + " |")
    print()
    rates = (0.0, 0.05, 0.10)
    print("| repeat period | " + " | ".join("T = %d, %d %% subst." % (T, round(100 * r)) for r in rates for T in SCORES) + " |")
    print("|---|" + "---|" * (len(SCORES) * len(rates)))
    for period in range(1, 21):
        cells = []
        for r in rates:
            cells += shares([model.repeat(rng, period, 4000, rate=r) for _ in range(16)])[1]
        print("| %d | " % period + " | ".join(cells) + " |")


if __name__ == "__main__":
    main()
