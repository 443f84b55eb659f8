#!/usr/bin/env python3
"""Time the contaminant screen with hashed K-mers (--exclude_k) over N reads resident in HBM, beside the 16-mer bitmap as the yardstick
(tools/bench_screen.py has the read set: filtlong_amd.synth.lengths, 10^5 reads are 0.998 Gbp):
  k16_<size>            flx_screen_hits_dev against a Kmers of random X: the existing path
  k<K>_<size>_share_<s> for K in --ks and X of --sizes bases of random sequence, with 0 % and 10 % of the reads drawn from X at 5 %
                        substitutions: flx_screenset_hits_dev; the bracket "flx_screen", the set's keys, capacity and bytes, the
                        hits and how many reads the 10 % threshold excludes
  build_<size>          for the largest X and K = 31: wall time of building the set in batches of 16 MiB, once with the capacity hinted
                        from the size and once grown from 16 slots; capacity and bytes of the table
  --ab LABEL            nothing of the above: the scoring step without the flag ("plain") and with the 16-mer screen against X of
                        5 kbp ("exclude16"), to be run alternately on this tree and, through FLX_LIB_PATH, on a build of the parent
                        commit; LABEL ("tree" / "parent") goes into the record
Medians of --steps runs behind a warm-up.  One JSON line on stdout, appended to --out (profiles/screen_k.jsonl) when given."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_screen import make_seq_plane, random_seq  # noqa: E402

BATCH = 16 << 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=100_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--ks", default="24,31")
    ap.add_argument("--sizes", default="5000,5000000,100000000")
    ap.add_argument("--shares", default="0,0.1")
    ap.add_argument("--ab", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from filtlong_amd import api, synth
    ctx = api.Context(0)
    L = ctx.L
    n = args.reads
    lengths = synth.lengths(n).astype(np.int32)
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

    def measure(call, d_seq, with_score=False):
        wall, screen = [], []
        for step in range(args.steps + 1):  # (the first is the warm-up)
            ctx.timing_reset()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if with_score:
                score()
            if call is not None:
                call(d_seq.data_ptr(), d_seq.numel(), d_off.data_ptr(), d_len.data_ptr(), d_ord.data_ptr(), n, d_hits.data_ptr())
            ctx.synchronize()
            w = (time.perf_counter() - t0) * 1e3
            if step:
                wall.append(w)
                screen.append(ctx.timing_get("flx_screen")[0])
        return {"wall_ms": stat(wall), "screen_ms": stat(screen)} if call is not None else {"wall_ms": stat(wall)}

    def result(m, size_of_set, k):
        hits = d_hits.cpu().numpy().astype(np.uint32)
        windows = np.maximum(0, lengths.astype(np.int64) - k + 1)
        t = api.screen_threshold(10.0)
        m.update(set_size=size_of_set, hits=int(hits.astype(np.int64).sum()),
                 excluded=int(((windows > 0) & ((hits.astype(np.uint64) << np.uint64(32)) >= np.uint64(t) * windows.astype(np.uint64))).sum()))
        return m

    def build(k, x, hint):
        ss = api.ScreenSet(ctx, k, hint)
        t0 = time.perf_counter()
        for a in range(0, len(x), BATCH):  # (a batch ends K - 1 bases into the next: no window is lost)
            ss.add_fasta([x[a:a + BATCH + k - 1].tobytes()])
        ss.finalize()
        return ss, (time.perf_counter() - t0) * 1e3

    ctx.timing_enable(True)
    rec = {"tool": "bench_screen_k", "time": time.strftime("%Y-%m-%dT%H:%M:%SZ", time.gmtime()), "device": ctx.device_info()["name"], "reads": n,
           "bases": int(lengths.astype(np.int64).sum()), "steps": args.steps, "library": os.environ.get("FLX_LIB_PATH", "tree")}
    base = random_seq(np.random.default_rng(3), pb.value)
    if args.ab:
        rec["label"] = args.ab
        rec["plain"] = measure(None, None, with_score=True)
        x = random_seq(np.random.default_rng(5000), 5000)
        plane, _ = make_seq_plane(base, lengths, offsets, np.random.default_rng(11), x, 0.1)
        d_seq = torch.from_numpy(plane).cuda()
        ks = api.Kmers(ctx)
        ks.add_screen_fasta([x.tobytes()])
        ks.finalize()
        rec["exclude16"] = measure(lambda *a: ctx.screen_hits_dev(ks, *a), d_seq, with_score=True)
        ks.close()
    else:
        sizes = [int(v) for v in args.sizes.split(",")]
        for size in sizes:
            x = random_seq(np.random.default_rng(size), size)
            hint = int(np.ceil(np.log2(2 * size)))
            for share in [float(v) for v in args.shares.split(",")]:
                plane, n_drawn = make_seq_plane(base, lengths, offsets, np.random.default_rng(11), x, share)
                d_seq = torch.from_numpy(plane).cuda()
                tag = "%d_share_%d" % (size, int(share * 100))
                ks = api.Kmers(ctx)
                ks.add_screen_fasta([x.tobytes()])
                ks.finalize()
                m = result(measure(lambda *a: ctx.screen_hits_dev(ks, *a), d_seq), len(ks), 16)
                m.update(filter=ctx.last_screen_filter(), drawn=n_drawn)
                rec["k16_" + tag] = m
                ks.close()
                for k in [int(v) for v in args.ks.split(",")]:
                    ss, _ = build(k, x, hint)
                    m = result(measure(lambda *a: ctx._check(L.flx_screenset_hits_dev(ctx.h, ss.h, *a)), d_seq), len(ss), k)
                    m.update(capacity=ss.capacity, table_bytes=8 * ss.capacity, drawn=n_drawn)
                    rec["k%d_%s" % (k, tag)] = m
                    ss.close()
                del d_seq
        size = max(sizes)
        x = random_seq(np.random.default_rng(size), size)
        for name, hint in (("hinted", int(np.ceil(np.log2(2 * size)))), ("grown", 4)):
            ss, ms = build(31, x, hint)
            rec["build_%d_%s" % (size, name)] = {"wall_ms": round(ms, 1), "set_size": len(ss), "capacity": ss.capacity, "table_bytes": 8 * ss.capacity}
            ss.close()
    ctx.timing_enable(False)
    line = json.dumps(rec, sort_keys=True)
    print(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
