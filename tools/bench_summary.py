#!/usr/bin/env python3
"""Time flx_summary_dev on N reads2 entries resident in HBM, beside the stage it follows and the host pass it replaces:
  summary_bracket_ms   the "flx_summary" timing bracket (HIP events: five kernels, their small copies and the host's digit choice
                       between them)
  summary_wall_ms      wall clock of the flx_summary_dev call
  rank_and_cut_ms      wall clock of flx_rank_and_cut_dev on the same arrays in the same run (target: half the bases)
  numpy_ms             a host sort-and-cumsum of the same arrays: descending sort of the lengths, cumulative sum, the nine Nx by
                       searchsorted, the three histograms by searchsorted + bincount
Lengths follow the benchmark's C2 configuration (filtlong_amd.synth.lengths: gamma(k = 4), mean 10 kbp).  One JSON line on stdout,
appended to --out (profiles/summary.jsonl) when given."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def host_numpy(ln, mq, wq, mask, edges):
    t0 = time.perf_counter()
    keep = mask != 0
    l64 = ln[keep].astype(np.int64)
    desc = np.sort(l64)[::-1]
    cum = np.cumsum(desc)
    bases = int(cum[-1])
    nx = [int(desc[np.searchsorted(cum, -(-x * bases // 100))]) for x in range(10, 100, 10)]
    b = np.searchsorted(2 ** np.arange(1, 32, dtype=np.int64), l64, side="right")
    np.bincount(b, minlength=32), np.bincount(b, weights=l64, minlength=32)
    for q in (mq[keep], wq[keep]):
        k = np.searchsorted(edges, q, side="right") - 1
        np.bincount(k, minlength=52), np.bincount(k, weights=l64, minlength=52)
    return (time.perf_counter() - t0) * 1e3, nx


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from filtlong_amd import api, synth
    ctx = api.Context(0)
    n = args.reads
    ln = synth.lengths(n)
    rng = np.random.RandomState(1)
    mq = rng.uniform(59, 99, n)
    wq = mq * rng.uniform(0.3, 1.0, n)
    passed0 = (rng.uniform(0, 1, n) > 0.1).astype(np.uint8)
    d_ln, d_mq, d_wq, d_p0 = (torch.from_numpy(a).cuda() for a in (ln, mq, wq, passed0))
    total = int(ln.astype(np.int64).sum())
    d_pass = d_p0.clone()
    torch.cuda.synchronize()

    def rank():
        d_pass.copy_(d_p0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ctx.rank_and_cut_dev(n, d_mq.data_ptr(), d_wq.data_ptr(), d_ln.data_ptr(), d_pass.data_ptr(), target_bases=total // 2, total_bases=total)
        return (time.perf_counter() - t0) * 1e3

    def summary():
        t0 = time.perf_counter()
        s = ctx.summary_dev(n, d_ln.data_ptr(), d_mq.data_ptr(), d_wq.data_ptr(), d_pass.data_ptr())
        return (time.perf_counter() - t0) * 1e3, s

    rank(), summary()  # warm-up
    ctx.timing_enable(True)
    rank_ms, wall_ms, bracket_ms = [], [], []
    for _ in range(args.steps):
        rank_ms.append(rank())
        ctx.timing_reset()
        w, s = summary()
        wall_ms.append(w)
        bracket_ms.append(ctx.timing_get("flx_summary")[0])
    ctx.timing_enable(False)
    np_ms, nx = host_numpy(ln, mq, wq, d_pass.cpu().numpy(), api.summary_q_edges())
    assert nx == s["nx"], (nx, s["nx"])
    rec = {"tool": "bench_summary", "time": time.strftime("%Y-%m-%dT%H:%M:%SZ", time.gmtime()), "device": ctx.device_info()["name"],
           "reads": n, "kept": s["n"], "kept_bases": s["bases"], "n50": s["nx"][4], "steps": args.steps,
           "summary_bracket_ms": {"median": round(float(np.median(bracket_ms)), 3), "best": round(min(bracket_ms), 3)},
           "summary_wall_ms": {"median": round(float(np.median(wall_ms)), 3), "best": round(min(wall_ms), 3)},
           "rank_and_cut_ms": {"median": round(float(np.median(rank_ms)), 3), "best": round(min(rank_ms), 3)},
           "numpy_ms": round(np_ms, 1)}
    line = json.dumps(rec, sort_keys=True)
    print(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
