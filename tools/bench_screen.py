#!/usr/bin/env python3
"""Time the contaminant screen (--exclude) over N reads resident in HBM, beside the Phred scoring step it runs behind:
  plain        flx_score_batch_dev over the quality plane: the step as it is WITHOUT the flag (--plain-only stops here; run it with
               FLX_LIB_PATH pointing at a build of the parent commit for the A/B comparison on the same machine)
  x_<size>     for X of 5 kbp, 50 kbp, 500 kbp and 5 Mbp of random sequence, with 0 % and with 10 % of the reads drawn from X at 5 %
               substitutions: the step with the flag (flx_score_batch_dev, then flx_screen_hits_dev over the sequence plane; wall clock),
               the screen's own bracket "flx_screen", the filter form that ran, how full the 10-mer table is, and how many reads the
               10 % threshold excludes.  --forms also runs every X with FLX_KMER_PREFILTER=12 (no LDS table) and =0 (bitmap alone);
               --fill-sweep runs every X with =12 and with =10 (the LDS table however full): the sweep the threshold of the LDS form
               is chosen from.
Lengths follow the benchmark's C2 configuration (filtlong_amd.synth.lengths: gamma(k = 4), mean 10 kbp: 10^5 reads are 0.998 Gbp);
--long-mbp M adds one read of M Mbp.  Medians of --steps runs behind a warm-up.  One JSON line on stdout, appended to --out
(profiles/screen.jsonl) when given."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def random_seq(rng, n):
    return ACGT[rng.integers(0, 4, size=n, dtype=np.uint8)]


def pre10_fill(x):
    """the share of the 4^10 10-mers that occur in x or its reverse complement: how full the screen's LDS table is"""
    c = np.searchsorted(ACGT, x).astype(np.uint32)
    seen = np.zeros(1 << 20, dtype=bool)
    for strand in (c, 3 - c[::-1]):
        v = np.zeros(len(strand) - 9, dtype=np.uint32)
        for k in range(10):
            v = (v << np.uint32(2)) | strand[k:len(strand) - 9 + k]
        seen[v] = True
    return round(float(seen.mean()), 4)


def make_seq_plane(base, lengths, offsets, rng, x, share):
    """the random reads of `base`; `share` of them are copies of stretches of x (either strand) with 5 % substitutions"""
    plane = base.copy()
    comp = np.zeros(256, dtype=np.uint8)
    comp[list(b"ACGT")] = list(b"TGCA")
    xr = comp[x[::-1]]
    drawn = np.flatnonzero(rng.random(len(lengths)) < share)
    for i in drawn:
        o, n = int(offsets[i]), int(lengths[i])
        at = 0
        while at < n:
            m = min(n - at, len(x))
            a = int(rng.integers(0, len(x) - m + 1))
            src = (xr if rng.integers(0, 2) else x)[a:a + m].copy()
            sub = np.flatnonzero(rng.random(m) < 0.05)
            src[sub] = ACGT[(np.searchsorted(ACGT, src[sub]) + rng.integers(1, 4, size=len(sub))) % 4]
            plane[o + at:o + at + m] = src
            at += m
    return plane, len(drawn)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=100_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--sizes", default="5000,50000,500000,5000000")
    ap.add_argument("--long-mbp", type=float, default=0.0)
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--forms", action="store_true")
    ap.add_argument("--fill-sweep", action="store_true")  # every X with the 12-mer form and with the LDS form forced (FLX_KMER_PREFILTER=12 / =10)
    ap.add_argument("--shares", default="0,0.1")
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
    d_pass, d_hits = torch.empty(n, dtype=torch.uint8, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda")
    d_qual = torch.from_numpy(rng.integers(25 + 33, 41 + 33, size=pb.value, dtype=np.uint8)).cuda()

    def stat(v):
        return {"median": round(float(np.median(v)), 3), "best": round(min(v), 3), "worst": round(max(v), 3)}

    def score():
        s = api.Scores()
        s.mean_q, s.window_q, s.passed = d_mean.data_ptr(), d_win.data_ptr(), d_pass.data_ptr()
        ctx._check(L.flx_score_batch_dev(ctx.h, None, d_qual.data_ptr(), d_qual.numel(), d_off.data_ptr(), d_len.data_ptr(), d_ord.data_ptr(), n,
                                         C.byref(params), C.byref(s)))

    def measure(ks, d_seq):
        wall, phred, screen = [], [], []
        for step in range(args.steps + 1):  # (the first is the warm-up)
            ctx.timing_reset()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            score()
            if ks is not None:
                ctx.screen_hits_dev(ks, d_seq.data_ptr(), d_seq.numel(), d_off.data_ptr(), d_len.data_ptr(), d_ord.data_ptr(), n, d_hits.data_ptr())
                ctx.synchronize()
            w = (time.perf_counter() - t0) * 1e3
            if step:
                wall.append(w)
                phred.append(ctx.timing_get("flx_score_phred")[0])
                screen.append(ctx.timing_get("flx_screen")[0])
        out = {"wall_ms": stat(wall), "phred_ms": stat(phred)}
        if ks is not None:
            out["screen_ms"] = stat(screen)
        return out

    ctx.timing_enable(True)
    rec = {"tool": "bench_screen", "label": args.label, "time": time.strftime("%Y-%m-%dT%H:%M:%SZ", time.gmtime()), "device": ctx.device_info()["name"],
           "reads": n, "bases": int(lengths.astype(np.int64).sum()), "steps": args.steps, "long_mbp": args.long_mbp,
           "library": os.environ.get("FLX_LIB_PATH", "tree")}
    rec["plain"] = measure(None, None)
    if not args.plain_only:
        rec["span"] = api.screen_span()
        base = random_seq(np.random.default_rng(3), pb.value)
        forms = [("", None)] + ([("_pre12", "12"), ("_exact", "0")] if args.forms else []) + ([("_pre12", "12"), ("_lds", "10")] if args.fill_sweep else [])
        for size in [int(v) for v in args.sizes.split(",")]:
            x = random_seq(np.random.default_rng(size), size)
            fill = pre10_fill(x)
            for share in [float(v) for v in args.shares.split(",")]:
                plane, n_drawn = make_seq_plane(base, lengths, offsets, np.random.default_rng(11), x, share)
                d_seq = torch.from_numpy(plane).cuda()
                for suffix, env in forms:
                    if env is None:
                        os.environ.pop("FLX_KMER_PREFILTER", None)
                    else:
                        os.environ["FLX_KMER_PREFILTER"] = env  # (read when the set is finalized)
                    ks = api.Kmers(ctx)
                    ks.add_screen_fasta([x.tobytes()])
                    ks.finalize()
                    m = measure(ks, d_seq)
                    hits = d_hits.cpu().numpy().astype(np.uint32)
                    m.update(filter=ctx.last_screen_filter(), set_size=len(ks), drawn=n_drawn, pre10_fill=fill,
                             excluded=int(api.screen_excluded(hits, lengths, 10.0).sum()), hits=int(hits.astype(np.int64).sum()))
                    rec["x_%d_share_%d%s" % (size, int(share * 100), suffix)] = m
                    ks.close()
                del d_seq
        os.environ.pop("FLX_KMER_PREFILTER", None)
    ctx.timing_enable(False)
    line = json.dumps(rec, sort_keys=True)
    print(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
