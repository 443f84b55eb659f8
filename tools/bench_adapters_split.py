#!/usr/bin/env python3
"""Time the search for adapters inside the reads (--split_adapters) over N reads resident in HBM, beside the steps it runs inside:
  plain        flx_score_batch_dev over the quality plane: the step WITHOUT any adapter flag
  trim         flx_score_batch_adapters_dev with the middle search off: the step with --trim_adapters alone (4 patterns)
               (--baseline-only stops here; run it with FLX_LIB_PATH pointing at a build of the parent commit for the A/B comparison on
               the same machine, alternately with this tree)
  p_<n>        for sets of n patterns (n / 2 random sequences of 28 bases) and 0 % and 1 % chimeras (an adapter in the middle of
               the read): flx_adapter_marks_dev alone (its bracket "flx_adapter_marks"), beside the derived estimate of about 40
               VALU instructions per (pattern, text base) at 3.9e13 lane-instructions a second, the warm-up of 96 bases per piece of
               1024 included, with the ratio; and the step WITH the flag (wall clock).
Lengths follow the benchmark's C2 configuration (filtlong_amd.synth.lengths: gamma(k = 4), mean 10 kbp: 10^5 reads are 0.998 Gbp).
Medians of --steps runs behind a warm-up.  One JSON line on stdout, appended to --out (profiles/adapters_split.jsonl) when given."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
LANE_INSTRUCTIONS_PER_S = 1024 * 16 * 2.4e9  # SIMDs x lanes x clock
VALU_PER_BASE = 40                            # derived, not measured: about 20 64-bit integer operations
PIECE, WARMUP = 1024, 96


def random_seq(rng, n):
    return ACGT[rng.integers(0, 4, size=n, dtype=np.uint8)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=100_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--patterns", default="4,40,256")
    ap.add_argument("--shares", default="0,0.01")
    ap.add_argument("--split_errors", type=int, default=10)
    ap.add_argument("--baseline-only", action="store_true")
    ap.add_argument("--label", default="")
    ap.add_argument("--library", default="this tree", help="what FLX_LIB_PATH holds, for the record (e.g. 'parent commit, built from its sources')")
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
    cap = 2 * n
    d_len, d_ord = torch.from_numpy(lengths).cuda(), torch.from_numpy(order.astype(np.int32)).cuda()
    d_off = torch.from_numpy(offsets.astype(np.int64)).cuda()
    d_mean, d_win = torch.empty(n, dtype=torch.float64, device="cuda"), torch.empty(n, dtype=torch.float64, device="cuda")
    d_pass = torch.empty(n, dtype=torch.uint8, device="cuda")
    d_first, d_last = torch.empty(n, dtype=torch.int32, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda")
    d_coff = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    d_crng = torch.empty(2 * cap, dtype=torch.int32, device="cuda")
    d_cmean, d_cwin = torch.empty(cap, dtype=torch.float64, device="cuda"), torch.empty(cap, dtype=torch.float64, device="cuda")
    d_cpass = torch.empty(cap, dtype=torch.uint8, device="cuda")
    d_marks = torch.empty((pb.value + 31) // 32, dtype=torch.int32, device="cuda")
    d_qual = torch.from_numpy(rng.integers(25 + 33, 41 + 33, size=pb.value, dtype=np.uint8)).cuda()

    def stat(v):
        return {"median": round(float(np.median(v)), 3), "best": round(min(v), 3), "worst": round(max(v), 3)}

    def scores(children):
        s = api.Scores()
        s.mean_q, s.window_q, s.passed = d_mean.data_ptr(), d_win.data_ptr(), d_pass.data_ptr()
        if children:
            s.first, s.last, s.child_offsets = d_first.data_ptr(), d_last.data_ptr(), d_coff.data_ptr()
            s.child_ranges, s.child_mean_q, s.child_window_q, s.child_passed = d_crng.data_ptr(), d_cmean.data_ptr(), d_cwin.data_ptr(), d_cpass.data_ptr()
            s.child_capacity = cap
        return s

    def measure(run, names):
        wall, brackets = [], {k: [] for k in names}
        for step in range(args.steps + 1):  # (the first is the warm-up)
            ctx.timing_reset()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run()
            ctx.synchronize()
            w = (time.perf_counter() - t0) * 1e3
            if step:
                wall.append(w)
                for k in names:
                    brackets[k].append(ctx.timing_get(k)[0])
        out = {"wall_ms": stat(wall)}
        out.update({k + "_ms": stat(v) for k, v in brackets.items()})
        return out

    def plain():
        s = scores(False)
        ctx._check(L.flx_score_batch_dev(ctx.h, None, d_qual.data_ptr(), d_qual.numel(), d_off.data_ptr(), d_len.data_ptr(), d_ord.data_ptr(), n,
                                         C.byref(params), C.byref(s)))

    def step_with(ad, d_seq):
        def step():
            s = scores(True)
            ctx._check(L.flx_score_batch_adapters_dev(ctx.h, ad.h, d_qual.data_ptr(), d_seq.data_ptr(), d_qual.numel(), d_off.data_ptr(),
                                                      d_len.data_ptr(), d_ord.data_ptr(), n, C.byref(params), C.byref(s)))
        return step

    ctx.timing_enable(True)
    rec = {"tool": "bench_adapters_split", "label": args.label, "time": time.strftime("%Y-%m-%dT%H:%M:%SZ", time.gmtime()),
           "device": ctx.device_info()["name"], "reads": n, "bases": int(lengths.astype(np.int64).sum()), "steps": args.steps,
           "split_errors": args.split_errors, "library": args.library}
    base = random_seq(np.random.default_rng(3), pb.value)
    d_base = torch.from_numpy(base).cuda()
    rec["plain"] = measure(plain, ["flx_score_phred"])
    trim_seqs = [random_seq(np.random.default_rng(4), 28).tobytes() for _ in range(2)]
    ad = api.Adapters(trim_seqs, errors=20, window=150)
    rec["trim"] = measure(step_with(ad, d_base), ["flx_adapters", "flx_score_phred"])
    ad.close()
    if not args.baseline_only:
        pieces = (lengths.astype(np.int64) + PIECE - 1) // PIECE
        text_bases = int(lengths.astype(np.int64).sum() + WARMUP * np.maximum(pieces - 1, 0).sum())
        for n_pat in [int(v) for v in args.patterns.split(",")]:
            srng = np.random.default_rng(n_pat)
            seqs = [random_seq(srng, 28).tobytes() for _ in range(n_pat // 2)]
            ad = api.Adapters(seqs, errors=20, window=150, split_errors=args.split_errors)
            estimate_ms = VALU_PER_BASE * n_pat * text_bases / LANE_INSTRUCTIONS_PER_S * 1e3
            for share in [float(v) for v in args.shares.split(",")]:
                plane = base.copy()
                prng = np.random.default_rng(11)
                drawn = np.flatnonzero((prng.random(n) < share) & (lengths > 1000))
                for i in drawn:  # an adapter in the middle of the read
                    o = int(offsets[i]) + int(lengths[i]) // 2
                    plane[o:o + 28] = np.frombuffer(seqs[int(prng.integers(0, len(seqs)))], dtype=np.uint8)
                d_seq = torch.from_numpy(plane).cuda()

                def marks():
                    ctx.adapter_marks_dev(ad, d_seq.data_ptr(), d_seq.numel(), d_off.data_ptr(), d_len.data_ptr(), d_ord.data_ptr(), n, d_marks.data_ptr())

                m = {"marks": measure(marks, ["flx_adapter_marks"])}
                m["step"] = measure(step_with(ad, d_seq), ["flx_adapters", "flx_adapter_marks", "flx_adapter_split", "flx_score_phred", "flx_qsplit_children"])
                per = np.diff(d_coff.cpu().numpy())
                m.update(drawn=int(len(drawn)), children=int(per.sum()), split_reads=int((per >= 2).sum()), estimate_ms=round(estimate_ms, 3),
                         measured_over_estimate=round(m["marks"]["flx_adapter_marks_ms"]["median"] / estimate_ms, 2))
                rec["p_%d_share_%g" % (n_pat, share * 100)] = m
                del d_seq
            ad.close()
    ctx.timing_enable(False)
    line = json.dumps(rec, sort_keys=True)
    print(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
