#!/usr/bin/env python3
"""Time one Phred scoring step over N reads resident in HBM without --split_window_q and with it:
  plain          flx_score_batch_dev, the step as it is without the flag (its code path is untouched by qsplit.hip)
  flag_no_split  flx_score_batch_qsplit_dev over the same reads, none of which has a bad window: the pure detection cost (the count
                 pass reads the quality plane a second time)
  flag_split     the same with a junk stretch of --junk bases in --share of the reads: count pass, emit pass, child plane, and the
                 children's scoring
Each with the wall clock of the call and the timing brackets "flx_score_phred" (all Phred kernels, parents and children),
"flx_qsplit_detect" (both passes) and "flx_qsplit_children" (layout and gather).  Lengths follow the benchmark's C2 configuration
(filtlong_amd.synth.lengths: gamma(k = 4), mean 10 kbp); qualities are made on the host, Phred 25-40 with Phred 0-3 stretches.
--long-mbp M adds one read of M Mbp to the batch (one wave walks it: the time of the slowest wave).  One JSON line on stdout,
appended to --out (profiles/qsplit.jsonl) when given."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make_plane(api, lengths, rng, share, junk):
    n = len(lengths)
    offsets = np.zeros(n, dtype=np.uint64)
    pb = C.c_uint64()
    assert api._lib.load().flx_plane_layout(lengths.ctypes.data, n, offsets.ctypes.data, C.byref(pb)) == 0
    good = rng.integers(25 + 33, 41 + 33, size=pb.value, dtype=np.uint8)
    plane = np.zeros(pb.value, dtype=np.uint8)
    split = rng.random(n) < share
    for i in range(n):
        o, l = int(offsets[i]), int(lengths[i])
        plane[o:o + l] = good[o:o + l]  # (the padding between the reads stays zero)
        if split[i] and l > 3 * junk:
            a = int(rng.integers(junk, l - 2 * junk))
            plane[o + a:o + a + junk] = rng.integers(33, 37, size=junk, dtype=np.uint8)
    return plane, offsets


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=100_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--window", type=int, default=250)
    ap.add_argument("--q", type=float, default=85.0)
    ap.add_argument("--share", type=float, default=0.10)
    ap.add_argument("--junk", type=int, default=500)
    ap.add_argument("--long-mbp", type=float, default=0.0)
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
    order = api.length_order(lengths)
    params = api.make_params(window_size=args.window)
    d_len, d_ord = torch.from_numpy(lengths).cuda(), torch.from_numpy(order.astype(np.int32)).cuda()
    d_mean, d_win = torch.empty(n, dtype=torch.float64, device="cuda"), torch.empty(n, dtype=torch.float64, device="cuda")
    d_pass, d_first, d_last = torch.empty(n, dtype=torch.uint8, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda")
    d_coff = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    cap = 4 * n
    d_crng, d_cmean = torch.empty(2 * cap, dtype=torch.int32, device="cuda"), torch.empty(cap, dtype=torch.float64, device="cuda")
    d_cwin, d_cpass = torch.empty(cap, dtype=torch.float64, device="cuda"), torch.empty(cap, dtype=torch.uint8, device="cuda")

    def scores():
        s = api.Scores()
        s.mean_q, s.window_q, s.passed, s.first, s.last = d_mean.data_ptr(), d_win.data_ptr(), d_pass.data_ptr(), d_first.data_ptr(), d_last.data_ptr()
        s.child_offsets, s.child_ranges, s.child_mean_q, s.child_window_q, s.child_passed = (d_coff.data_ptr(), d_crng.data_ptr(), d_cmean.data_ptr(),
                                                                                             d_cwin.data_ptr(), d_cpass.data_ptr())
        s.child_capacity = cap
        return s

    def measure(d_plane, d_off, flag):
        wall, phred, detect, children, nc = [], [], [], [], 0
        for step in range(args.steps + 1):  # (the first is the warm-up)
            s = scores()
            ctx.timing_reset()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if flag:
                ctx._check(L.flx_score_batch_qsplit_dev(ctx.h, d_plane.data_ptr(), d_plane.numel(), d_off.data_ptr(), d_len.data_ptr(), d_ord.data_ptr(), n,
                                                        C.byref(params), args.q, C.byref(s)))
            else:
                ctx._check(L.flx_score_batch_dev(ctx.h, None, d_plane.data_ptr(), d_plane.numel(), d_off.data_ptr(), d_len.data_ptr(), d_ord.data_ptr(), n,
                                                 C.byref(params), C.byref(s)))
            w = (time.perf_counter() - t0) * 1e3
            if step:
                wall.append(w)
                phred.append(ctx.timing_get("flx_score_phred")[0])
                detect.append(ctx.timing_get("flx_qsplit_detect")[0])
                children.append(ctx.timing_get("flx_qsplit_children")[0])
            nc = int(s.n_children)

        def stat(v):
            return {"median": round(float(np.median(v)), 3), "best": round(min(v), 3)}
        return {"wall_ms": stat(wall), "phred_ms": stat(phred), "detect_ms": stat(detect), "children_ms": stat(children), "children": nc}

    ctx.timing_enable(True)
    rec = {"tool": "bench_qsplit", "time": time.strftime("%Y-%m-%dT%H:%M:%SZ", time.gmtime()), "device": ctx.device_info()["name"], "reads": n,
           "bases": int(lengths.astype(np.int64).sum()), "window": args.window, "q": args.q, "steps": args.steps, "long_mbp": args.long_mbp}
    for name, share in (("no_split", 0.0), ("split", args.share)):
        plane, offsets = make_plane(api, lengths, np.random.default_rng(7), share, args.junk)
        d_plane, d_off = torch.from_numpy(plane).cuda(), torch.from_numpy(offsets.astype(np.int64)).cuda()
        if name == "no_split":
            rec["plain"] = measure(d_plane, d_off, False)
        rec["flag_" + name] = measure(d_plane, d_off, True)
        if name == "split":
            rec["plain_on_split_data"] = measure(d_plane, d_off, False)
            rec["share"], rec["junk"] = share, args.junk
        del d_plane, d_off
    assert rec["flag_no_split"]["children"] == 0 and rec["flag_split"]["children"] > 0
    ctx.timing_enable(False)
    line = json.dumps(rec, sort_keys=True)
    print(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
