#!/usr/bin/env python3
"""Time the low-complexity filter (--max_low_complexity) over N reads resident in HBM, beside the Phred scoring step it runs behind:
  plain        flx_score_batch_dev over the quality plane: the step as it is WITHOUT the flag (--plain-only stops here; run it with
               FLX_LIB_PATH pointing at a build of the parent commit for the A/B comparison on the same machine)
  random       the step with the flag (flx_score_batch_dev, then flx_complexity_bad_dev over a sequence plane of random bases; wall
               clock), the filter's own bracket "flx_complexity", the bad windows and the reads flagged at 50 %
  junk_<p>     the same with p % of the reads turned into repeats of period 1..6 (3 % substitutions): the counters then collide on
               few triplet kinds
  alone        flx_complexity_bad_dev without the scoring in front of it
Lengths follow the benchmark's C2 configuration (filtlong_amd.synth.lengths: gamma(k = 4), mean 10 kbp: 10^5 reads are 0.998 Gbp);
--long-mbp M adds one read of M Mbp.  Medians of --steps runs behind a warm-up.  One JSON line on stdout, appended to --out
(profiles/complexity.jsonl) when given."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def make_seq_plane(base, lengths, offsets, rng, share):
    """the random reads of `base`; `share` of them are repeats of period 1..6 with 3 % substitutions"""
    plane = base.copy()
    drawn = np.flatnonzero(rng.random(len(lengths)) < share)
    for i in drawn:
        o, n = int(offsets[i]), int(lengths[i])
        unit = ACGT[rng.integers(0, 4, size=int(rng.integers(1, 7)))]
        src = np.tile(unit, n // len(unit) + 1)[:n].copy()
        sub = np.flatnonzero(rng.random(n) < 0.03)
        src[sub] = ACGT[(np.searchsorted(ACGT, src[sub]) + rng.integers(1, 4, size=len(sub))) % 4]
        plane[o:o + n] = src
    return plane, len(drawn)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=100_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--long-mbp", type=float, default=0.0)
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--shares", default="0,0.1")
    ap.add_argument("--score", type=int, default=20)
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from filtlong_amd import api, synth
    ctx = api.Context(0)
    L = ctx.L
    n = args.reads
    lengths = synth.lengths(n).astype(np.int32)
    if args.long_mbp > 0:
        lengths = np.concatenate((lengths, np.array([int(args.long_mbp * 1e6)], dtype=np.int32)))
        n += 1
    offsets = np.zeros(n, dtype=np.uint64)
    pb = C.c_uint64()
    assert L.flx_plane_layout(lengths.ctypes.data, n, offsets.ctypes.data, C.byref(pb)) == 0
    order = api.length_order(lengths)
    params = api.make_params(window_size=250)
    rng = np.random.default_rng(7)
    d_len, d_ord = torch.from_numpy(lengths).cuda(), torch.from_numpy(order.astype(np.int32)).cuda()
    d_off = torch.from_numpy(offsets.astype(np.int64)).cuda()
    d_mean, d_win = torch.empty(n, dtype=torch.float64, device="cuda"), torch.empty(n, dtype=torch.float64, device="cuda")
    d_pass, d_bad = torch.empty(n, dtype=torch.uint8, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda")
    d_qual = torch.from_numpy(rng.integers(25 + 33, 41 + 33, size=pb.value, dtype=np.uint8)).cuda()

    def stat(v):
        return {"median": round(float(np.median(v)), 3), "best": round(min(v), 3), "worst": round(max(v), 3)}

    def score():
        s = api.Scores()
        s.mean_q, s.window_q, s.passed = d_mean.data_ptr(), d_win.data_ptr(), d_pass.data_ptr()
        ctx._check(L.flx_score_batch_dev(ctx.h, None, d_qual.data_ptr(), d_qual.numel(), d_off.data_ptr(), d_len.data_ptr(), d_ord.data_ptr(), n,
                                         C.byref(params), C.byref(s)))

    def measure(d_seq, with_score=True):
        wall, phred, filt = [], [], []
        for step in range(args.steps + 1):  # (the first is the warm-up)
            ctx.timing_reset()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if with_score:
                score()
            if d_seq is not None:
                ctx.complexity_bad_dev(d_seq.data_ptr(), d_seq.numel(), d_off.data_ptr(), d_len.data_ptr(), d_ord.data_ptr(), n, args.score,
                                       d_bad.data_ptr())
            ctx.synchronize()
            w = (time.perf_counter() - t0) * 1e3
            if step:
                wall.append(w)
                phred.append(ctx.timing_get("flx_score_phred")[0])
                filt.append(ctx.timing_get("flx_complexity")[0])
        out = {"wall_ms": stat(wall)}
        if with_score:
            out["phred_ms"] = stat(phred)
        if d_seq is not None:
            out["complexity_ms"] = stat(filt)
        return out

    ctx.timing_enable(True)
    rec = {"tool": "bench_complexity", "label": args.label, "time": time.strftime("%Y-%m-%dT%H:%M:%SZ", time.gmtime()),
           "device": ctx.device_info()["name"], "reads": n, "bases": int(lengths.astype(np.int64).sum()), "steps": args.steps,
           "long_mbp": args.long_mbp, "score": args.score, "library": os.environ.get("FLX_LIB_PATH", "tree")}
    rec["plain"] = measure(None)
    if not args.plain_only:
        rec["span"], rec["window"] = api.complexity_span(), api.complexity_window()
        base = ACGT[np.random.default_rng(3).integers(0, 4, size=pb.value, dtype=np.uint8)]
        for share in [float(v) for v in args.shares.split(",")]:
            plane, n_drawn = make_seq_plane(base, lengths, offsets, np.random.default_rng(11), share)
            d_seq = torch.from_numpy(plane).cuda()
            m = measure(d_seq)
            bad = d_bad.cpu().numpy().astype(np.uint32)
            m.update(drawn=n_drawn, bad_windows=int(bad.astype(np.int64).sum()), flagged=int(api.complexity_flagged(bad, lengths, 50.0).sum()))
            m["alone"] = measure(d_seq, with_score=False)
            rec["random" if share == 0 else "junk_%d" % int(share * 100)] = m
            del d_seq
    ctx.timing_enable(False)
    line = json.dumps(rec, sort_keys=True)
    print(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
