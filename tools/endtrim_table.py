#!/usr/bin/env python3
"""What --trim_ends_q cuts and what it leaves, from the model of the tests (tests/_endtrim_model.py; no GPU, the library only hands over
its table E): the mean number of bases cut per end at Q = 80, 90 and 95
  ramp R    for 400 reads of 5 kbp whose body has per-base qualities drawn uniformly from Q12..Q30 and whose two ends ramp up to
            that from Q2 over R = 0, 50 and 200 bases (each base jittered by up to 2), with the share of reads left without a base
  flat q    for reads of 5 kbp of one quality q at every base: a read is untouched or gone, and Q decides which
printed as the Markdown tables of README.md."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _endtrim_model as model  # noqa: E402

QS = (80, 90, 95)
LENGTH, READS = 5000, 400


def ramp_read(rng, ramp):
    q = rng.integers(12, 31, size=LENGTH)
    if ramp:
        up = 2 + (np.arange(ramp) * (21 - 2)) // ramp + rng.integers(-2, 3, size=ramp)
        q[:ramp] = np.clip(up, 0, 40)
        q[LENGTH - ramp:] = np.clip(up[::-1] + rng.integers(-2, 3, size=ramp), 0, 40)
    return (q + 33).astype(np.uint8).tobytes()


def main():
    from filtlong_amd import api
    rng = np.random.default_rng(2026)
    print("| ends | " + " | ".join("cut per end at Q = %d | reads gone" % Q for Q in QS) + " |")
    print("|---|" + "---|---|" * len(QS))
    for ramp in (0, 50, 200):
        reads = [ramp_read(rng, ramp) for _ in range(READS)]
        cells = []
        for Q in QS:
            cuts = model.batch_cuts(reads, api.qsplit_threshold(Q)).astype(np.int64)
            gone = (cuts[:, 0] + cuts[:, 1] >= LENGTH)
            kept = cuts[~gone]
            cells += ["%.1f" % kept.mean() if len(kept) else "-", "%.1f %%" % (100.0 * gone.mean())]
        print("| ramp of %d bases | " % ramp + " | ".join(cells) + " |")
    print()
    print("| flat quality | " + " | ".join("Q = %d" % Q for Q in QS) + " |")
    print("|---|" + "---|" * len(QS))
    for q in (5, 7, 10, 13, 20):
        read = bytes([q + 33]) * LENGTH
        cells = []
        for Q in QS:
            h, c = model.cuts(read, api.qsplit_threshold(Q))
            cells.append("untouched" if (h, c) == (0, 0) else "gone" if h + c >= LENGTH else "%d + %d" % (h, c))
        print("| Q%d at every base | " % q + " | ".join(cells) + " |")


if __name__ == "__main__":
    main()
