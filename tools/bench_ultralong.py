#!/usr/bin/env python3
"""Ultra-long reads in Phred mode: what 100 reads of 0.5-4 Mbp add to a C2-shaped scoring step, with the cooperative long-read path
(score_phred_long.hip) and without it (FLX_PHRED_LONG_MIN=0: every read in one lane of the default kernel), and one 4 Mbp read alone.

    python tools/bench_ultralong.py [--reads 1000000] [--steps 5] [--warmup 2] [--junk 0.03] [--centre 5,3] [--out FILE]

The batch: --reads reads from flx_synth_qual_dev with C2's length distribution (filtlong_amd/synth.py), in descending length order,
window size 250; the extra reads: ONT-like quality runs from numpy (seeded).  Time per step: score_reads_dev + device synchronise,
median over --steps after --warmup.  Prints one JSON line per row and a summary; --out also writes them to FILE.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def ont_qual(L, seed, junk=0.03, centre=(5.0, 3.0)):
    """runs of 300 bases around a gamma-distributed Phred centre, per-base noise; a share `junk` of the runs at Phred 0-3"""
    rng = np.random.default_rng(seed)
    run = 300
    seg = rng.gamma(centre[0], centre[1], L // run + 2).astype(np.float32)
    low = rng.random(len(seg)) < junk
    seg[low] = rng.uniform(0.0, 3.0, int(low.sum()))
    q = np.repeat(seg, run)[:L] + rng.standard_normal(L, dtype=np.float32) * np.float32(4.0)
    return (np.clip(np.rint(q), 0, 60) + 33).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--extra", type=int, default=100, help="ultra-long reads added to the batch")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--window-size", type=int, default=250)
    ap.add_argument("--junk", type=float, default=0.03,
                    help="share of 300-base runs of the extra reads at Phred 0-3 (windows around quality 0.5: the serial case)")
    ap.add_argument("--centre", default="5,3", help="gamma shape,scale of the runs' Phred centres (5,3: mean 15; 9,1.8: mean 16, fewer low runs)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch
    from filtlong_amd import api, synth

    ctx = api.Context(0)
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(2024)
    extra_lens = rng.integers(500_000, 4_000_001, args.extra).astype(np.int32)
    centre = tuple(float(x) for x in args.centre.split(","))
    extra = [ont_qual(int(L), 7000 + i, args.junk, centre) for i, L in enumerate(extra_lens)]
    params = api.make_params(window_size=args.window_size)
    rows = []

    def setup(lengths_base, extra_q):
        n0 = len(lengths_base)
        lengths = np.concatenate([lengths_base, np.array([len(x) for x in extra_q], dtype=np.int32)]).astype(np.int32)
        n = len(lengths)
        offsets = np.zeros(n, dtype=np.uint64)
        pb = C.c_uint64()
        ctx.L.flx_plane_layout(lengths.ctypes.data, n, offsets.ctypes.data, C.byref(pb))
        d_plane = torch.zeros(pb.value, dtype=torch.uint8, device=dev)
        d_off = torch.from_numpy(offsets.view(np.int64)).to(dev)
        d_len = torch.from_numpy(lengths).to(dev)
        if n0:
            d_ids = torch.arange(0, n0, dtype=torch.int64, device=dev)
            ctx.synth_qual_dev(synth.SEED, d_plane.data_ptr(), pb.value, d_off.data_ptr(), d_len.data_ptr(), d_ids.data_ptr(), n0)
        for i, q in enumerate(extra_q):
            o = int(offsets[n0 + i])
            d_plane[o:o + len(q)].copy_(torch.from_numpy(q))
        d_ord = torch.from_numpy(api.length_order(lengths).view(np.int32)).to(dev)
        outs = [torch.empty(n, dtype=torch.float64, device=dev), torch.empty(n, dtype=torch.float64, device=dev),
                torch.empty(n, dtype=torch.uint8, device=dev)]
        torch.cuda.synchronize()
        return dict(n=n, bases=int(lengths.astype(np.int64).sum()), plane=d_plane, pb=pb.value, off=d_off, len=d_len, ord=d_ord,
                    outs=outs)

    def run(name, b, long_min):
        if long_min is None:
            os.environ.pop("FLX_PHRED_LONG_MIN", None)
        else:
            os.environ["FLX_PHRED_LONG_MIN"] = str(long_min)

        def once():
            ctx.score_reads_dev(b["plane"].data_ptr(), b["pb"], b["off"].data_ptr(), b["len"].data_ptr(), b["ord"].data_ptr(), b["n"],
                                params, b["outs"][0].data_ptr(), b["outs"][1].data_ptr(), b["outs"][2].data_ptr())

        for _ in range(args.warmup):
            once()
        ts, long_ms = [], []
        for _ in range(args.steps):
            ctx.timing_enable(True)
            ctx.timing_reset()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            once()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
            long_ms.append(ctx.timing_get("flx_score_phred_long")[0])
            ctx.timing_enable(False)
        res = b["outs"][0].cpu().numpy().view(np.uint64).copy(), b["outs"][1].cpu().numpy().view(np.uint64).copy()
        row = {"row": name, "reads": b["n"], "bases": b["bases"], "FLX_PHRED_LONG_MIN": long_min, "ms_per_step": round(float(np.median(ts)), 3),
               "ms_min": round(min(ts), 3), "ms_max": round(max(ts), 3), "long_path_ms": round(float(np.median(long_ms)), 3),
               "kernel": ctx.last_phred_kernel()}
        print(json.dumps(row), flush=True)
        rows.append(row)
        return row, res

    lens = synth.lengths(args.reads)
    base = setup(lens, [])
    r_base, _ = run("c2_shape", base, None)
    r_base_off, _ = run("c2_shape", base, 0)
    del base
    torch.cuda.empty_cache()
    withx = setup(lens, extra)
    r_x, res_x = run("c2_shape+%d_ultralong" % args.extra, withx, None)
    r_x_off, res_x_off = run("c2_shape+%d_ultralong" % args.extra, withx, 0)
    same_x = all((a == b).all() for a, b in zip(res_x, res_x_off))
    del withx
    torch.cuda.empty_cache()
    one = setup(np.zeros(0, dtype=np.int32), [ont_qual(4_000_000, 99, args.junk, centre)])
    r_one, res_one = run("one_4mbp_read", one, None)
    r_one_off, res_one_off = run("one_4mbp_read", one, 0)
    same_one = all((a == b).all() for a, b in zip(res_one, res_one_off))
    os.environ.pop("FLX_PHRED_LONG_MIN", None)

    summary = {
        "summary": "ultra-long reads, Phred mode, window %d; extra reads: junk %.3f, centre gamma(%s)" % (args.window_size, args.junk, args.centre),
        "device": ctx.device_info()["name"],
        "c2_shape_ms": r_base["ms_per_step"],
        "with_ultralong_ms": r_x["ms_per_step"],
        "with_ultralong_ratio": round(r_x["ms_per_step"] / r_base["ms_per_step"], 3),
        "with_ultralong_path_off_ms": r_x_off["ms_per_step"],
        "with_ultralong_path_off_ratio": round(r_x_off["ms_per_step"] / r_base_off["ms_per_step"], 3),
        "one_4mbp_ms": r_one["ms_per_step"],
        "one_4mbp_path_off_ms": r_one_off["ms_per_step"],
        "same_bits_with_and_without_the_path": bool(same_x and same_one),
    }
    print(json.dumps(summary), flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            for r in rows + [summary]:
                fh.write(json.dumps(r) + "\n")
    ctx.close()
    return 0 if summary["same_bits_with_and_without_the_path"] else 1


if __name__ == "__main__":
    sys.exit(main())
