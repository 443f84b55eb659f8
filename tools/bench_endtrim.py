#!/usr/bin/env python3
"""Time the quality trimming of the read ends (--trim_ends_q) over N reads resident in HBM, beside the Phred scoring step it runs in
front of:
  plain        flx_score_batch_dev over the quality plane: the step as it is WITHOUT the flag (--plain-only stops here; run it with
               FLX_LIB_PATH pointing at a build of the parent commit for the A/B comparison on the same machine)
  alone        flx_endtrim_cuts_dev alone: its bracket "flx_endtrim" (the segment table, the span kernel, the per-read combine) and the
               wall clock, with the share of the HBM roofline (one byte a base at 6.3 TB/s) the bracket comes to
  trimmed      the step with the flag (flx_score_batch_endtrim_dev: the cuts, the child CSR, the parents' scoring, the child plane, the
               children's scoring; wall clock), its brackets, the reads cut and the children
The qualities are uniform Q25..Q40 with junk (Q0..Q9) of 0 to 120 bases at either end of two reads in three.  Lengths follow the
benchmark's C2 configuration (filtlong_amd.synth.lengths: gamma(k = 4), mean 10 kbp: 10^5 reads are 0.998 Gbp); --long-mbp M adds one
read of M Mbp.  Medians of --steps runs behind a warm-up.  One JSON line on stdout, appended to --out (profiles/endtrim.jsonl) when
given."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HBM_BYTES_PER_S = 6.3e12  # what a streaming read achieves on the MI355X


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=100_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--long-mbp", type=float, default=0.0)
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--q", type=float, default=90.0)
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
    plane = rng.integers(25 + 33, 41 + 33, size=pb.value, dtype=np.uint8)
    junk = rng.integers(33, 43, size=1 << 16, dtype=np.uint8)
    for i in range(n):
        if i % 3 == 2:
            continue
        o, ln = int(offsets[i]), int(lengths[i])
        h, c = (min(ln, int(v)) for v in rng.integers(0, 121, size=2))
        a = int(rng.integers(0, (1 << 16) - 256))
        plane[o:o + h] = junk[a:a + h]
        plane[o + ln - c:o + ln] = junk[a + 128:a + 128 + c]
    d_len, d_ord = torch.from_numpy(lengths).cuda(), torch.from_numpy(order.astype(np.int32)).cuda()
    d_off = torch.from_numpy(offsets.astype(np.int64)).cuda()
    d_mean, d_win = torch.empty(n, dtype=torch.float64, device="cuda"), torch.empty(n, dtype=torch.float64, device="cuda")
    d_pass, d_cuts = torch.empty(n, dtype=torch.uint8, device="cuda"), torch.empty(2 * n, dtype=torch.int32, device="cuda")
    d_first, d_last = torch.empty(n, dtype=torch.int32, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda")
    d_coff = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    d_crng = torch.empty(2 * n, dtype=torch.int32, device="cuda")
    d_cmean, d_cwin = torch.empty(n, dtype=torch.float64, device="cuda"), torch.empty(n, dtype=torch.float64, device="cuda")
    d_cpass = torch.empty(n, dtype=torch.uint8, device="cuda")
    d_qual = torch.from_numpy(plane).cuda()
    t = api.qsplit_threshold(args.q)
    bases = int(lengths.astype(np.int64).sum())

    def stat(v):
        return {"median": round(float(np.median(v)), 3), "best": round(min(v), 3), "worst": round(max(v), 3)}

    def scores(children):
        s = api.Scores()
        s.mean_q, s.window_q, s.passed = d_mean.data_ptr(), d_win.data_ptr(), d_pass.data_ptr()
        if children:
            s.first, s.last, s.child_offsets = d_first.data_ptr(), d_last.data_ptr(), d_coff.data_ptr()
            s.child_ranges, s.child_mean_q, s.child_window_q, s.child_passed = d_crng.data_ptr(), d_cmean.data_ptr(), d_cwin.data_ptr(), d_cpass.data_ptr()
            s.child_capacity = n
        return s

    def plain():
        s = scores(False)
        ctx._check(L.flx_score_batch_dev(ctx.h, None, d_qual.data_ptr(), d_qual.numel(), d_off.data_ptr(), d_len.data_ptr(), d_ord.data_ptr(), n,
                                         C.byref(params), C.byref(s)))

    def alone():
        ctx.endtrim_cuts_dev(d_qual.data_ptr(), d_qual.numel(), d_off.data_ptr(), d_len.data_ptr(), d_ord.data_ptr(), n, t, d_cuts.data_ptr())

    kids = [0]

    def trimmed():
        s = scores(True)
        ctx._check(L.flx_score_batch_endtrim_dev(ctx.h, d_qual.data_ptr(), d_qual.numel(), d_off.data_ptr(), d_len.data_ptr(), d_ord.data_ptr(), n,
                                                 C.byref(params), t, C.byref(s)))
        kids[0] = int(s.n_children)

    def measure(fn, brackets):
        wall, got = [], {b: [] for b in brackets}
        for step in range(args.steps + 1):  # (the first is the warm-up)
            ctx.timing_reset()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            ctx.synchronize()
            w = (time.perf_counter() - t0) * 1e3
            if step:
                wall.append(w)
                for b in brackets:
                    got[b].append(ctx.timing_get(b)[0])
        out = {"wall_ms": stat(wall)}
        out.update({b.replace("flx_", "").replace(".", "_") + "_ms": stat(v) for b, v in got.items()})
        return out

    ctx.timing_enable(True)
    rec = {"tool": "bench_endtrim", "label": args.label, "time": time.strftime("%Y-%m-%dT%H:%M:%SZ", time.gmtime()),
           "device": ctx.device_info()["name"], "reads": n, "bases": bases, "steps": args.steps, "long_mbp": args.long_mbp, "q": args.q,
           "library": os.environ.get("FLX_LIB_PATH", "tree")}
    rec["plain"] = measure(plain, ["flx_score_phred"])
    if not args.plain_only:
        rec["span"] = api.endtrim_span()
        rec["alone"] = measure(alone, ["flx_endtrim"])
        floor_ms = bases / HBM_BYTES_PER_S * 1e3
        rec["alone"]["hbm_floor_ms"] = round(floor_ms, 4)
        rec["alone"]["share_of_hbm_roofline"] = round(floor_ms / rec["alone"]["endtrim_ms"]["median"], 3)
        cuts = d_cuts.cpu().numpy().astype(np.uint32).reshape(-1, 2)
        rec["reads_cut"] = int((cuts != 0).any(axis=1).sum())
        rec["bases_cut"] = int(cuts.astype(np.int64).sum())
        rec["trimmed"] = measure(trimmed, ["flx_endtrim", "flx_score_phred", "flx_qsplit_children.layout", "flx_qsplit_children.gather"])
        rec["children"] = kids[0]
    ctx.timing_enable(False)
    line = json.dumps(rec, sort_keys=True)
    print(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
