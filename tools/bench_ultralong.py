#!/usr/bin/env python3
"""Ultra-long reads.  With --kmer: k-mer mode (see main_kmer below).  Without: Phred mode: what 100 reads of 0.5-4 Mbp add to a C2-shaped scoring step, with the cooperative long-read path
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
    ap.add_argument("--kmer", action="store_true", help="k-mer mode: the cooperative folds of score_kmer_long.hip against FLX_KMER_LONG_MIN=0")
    ap.add_argument("--crossover", action="store_true", help="--kmer: also one read of 2^16 .. 2^22 bases alone, with and without the paths, and "
                    "the cover path's spans per segment (8 .. 128) on one 4 Mbp read")
    ap.add_argument("--ultralong-only", type=int, default=2000, help="--kmer: reads of the ultralong_only row (0.1-4 Mbp each, nothing else; 0: no such row)")
    args = ap.parse_args()
    if args.kmer:
        return main_kmer(args)

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


def main_kmer(args):
    """k-mer mode (window 250, reference: 5 Mbp of random bases as an assembly).  Rows, each with both cooperative paths (default
    thresholds), with the cover path off (FLX_KMER_COVER_LONG_MIN=0) and with the folds' path off as well (FLX_KMER_LONG_MIN=0), plain
    and with --trim --split 500:
      * a C3-shaped step of --reads reads plus --extra reads of 0.5-4 Mbp (tiled from the reference, 3 % substitutions, junk blocks);
      * one 4 Mbp read alone;  ultralong_only: --ultralong-only reads of 0.1-4 Mbp and nothing else (synthesised on the device);
      * with --crossover one read of 2^16 .. 2^22 bases alone, and one 4 Mbp read at 8 .. 128 spans per segment of the cover path.
    Per row the device time of flx_score_kmer_cover (the whole stage), flx_score_kmer_cover.long (its segment launches),
    flx_score_kmer_fold and flx_score_kmer_long (medians over --steps), the wall time per step, and the words the folds' path replayed in
    floating point (from the FLX_API_TIMING stage line)."""
    import re
    import tempfile
    import torch
    from filtlong_amd import api, synth, _lib

    ctx = api.Context(0)
    dev = torch.device("cuda", 0)
    ref_len = 5_000_000
    ref = synth.bases_read(synth.STREAM_REF, 0, 0, ref_len)
    ks = api.Kmers(ctx)
    ks.add_assembly_fasta([ref.tobytes()])
    ks.finalize()
    d_ref = torch.from_numpy(ref).to(dev)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    rows = []

    def long_read(L, seed):
        rng = np.random.default_rng(seed)
        parts, have = [], 0
        while have < L:
            n = int(rng.integers(20_000, 150_000))
            a = int(rng.integers(0, ref_len - n))
            parts.append(ref[a:a + n])
            have += n
        seq = np.concatenate(parts)[:L].copy()
        sub = rng.random(L) < 0.03
        seq[sub] = acgt[rng.integers(0, 4, int(sub.sum()))]
        for _ in range(L // 100_000):
            n = int(rng.choice([40, 300, 600, 3000]))
            a = int(rng.integers(0, L - n))
            seq[a:a + n] = acgt[rng.integers(0, 4, n)]
        return seq

    def setup(lengths_base, extra):
        n0 = len(lengths_base)
        lengths = np.concatenate([lengths_base, np.array([len(x) for x in extra], dtype=np.int32)]).astype(np.int32)
        n = len(lengths)
        offsets = np.zeros(n, dtype=np.uint64)
        pb = C.c_uint64()
        ctx.L.flx_plane_layout(lengths.ctypes.data, n, offsets.ctypes.data, C.byref(pb))
        d_plane = torch.zeros(pb.value, dtype=torch.uint8, device=dev)
        d_off = torch.from_numpy(offsets.view(np.int64)).to(dev)
        d_len = torch.from_numpy(lengths).to(dev)
        if n0:
            d_ids = torch.arange(0, n0, dtype=torch.int64, device=dev)
            ctx.synth_seq_dev(synth.SEED, d_plane.data_ptr(), pb.value, d_off.data_ptr(), d_len.data_ptr(), d_ids.data_ptr(), n0, d_ref.data_ptr(), ref_len)
        for i, q in enumerate(extra):
            o = int(offsets[n0 + i])
            d_plane[o:o + len(q)].copy_(torch.from_numpy(q))
        d_ord = torch.from_numpy(api.length_order(lengths).view(np.int32)).to(dev)
        cap = 4 * n + 100_000
        t = {k: torch.zeros(sz, dtype=dt, device=dev) for k, sz, dt in (
            ("mean", n, torch.float64), ("win", n, torch.float64), ("pass", n, torch.uint8), ("first", n, torch.int32), ("last", n, torch.int32),
            ("coff", n + 1, torch.int64), ("crng", 2 * cap, torch.int32), ("cmean", cap, torch.float64), ("cwin", cap, torch.float64),
            ("cpass", cap, torch.uint8))}
        sc = _lib.Scores()
        sc.mean_q, sc.window_q, sc.passed, sc.first, sc.last = (t["mean"].data_ptr(), t["win"].data_ptr(), t["pass"].data_ptr(),
                                                               t["first"].data_ptr(), t["last"].data_ptr())
        sc.child_offsets, sc.child_ranges, sc.child_mean_q, sc.child_window_q, sc.child_passed = (
            t["coff"].data_ptr(), t["crng"].data_ptr(), t["cmean"].data_ptr(), t["cwin"].data_ptr(), t["cpass"].data_ptr())
        sc.child_capacity = cap
        torch.cuda.synchronize()
        return dict(n=n, bases=int(lengths.astype(np.int64).sum()), plane=d_plane, pb=pb.value, off=d_off, len=d_len, ord=d_ord, t=t, sc=sc)

    def run(name, b, children, long_min, steps=None, cover_min=None, spans=None):
        steps = steps or args.steps
        for key, value in (("FLX_KMER_LONG_MIN", long_min), ("FLX_KMER_COVER_LONG_MIN", cover_min), ("FLX_KMER_COVER_LONG_SPANS", spans)):
            if value is None:
                os.environ.pop(key, None)
            else:
                os.environ[key] = str(value)
        params = api.make_params(window_size=args.window_size, trim=children, split=500 if children else None)

        def once():
            ctx.score_kmer_dev(ks, b["plane"].data_ptr(), b["pb"], b["off"].data_ptr(), b["len"].data_ptr(), b["ord"].data_ptr(), b["n"], params, b["sc"])
            torch.cuda.synchronize()

        # one call with the stage line on: the library writes it to file descriptor 2
        replayed = None
        with tempfile.TemporaryFile() as tmp:
            saved = os.dup(2)
            os.environ["FLX_API_TIMING"] = "1"
            os.dup2(tmp.fileno(), 2)
            try:
                once()
            finally:
                os.dup2(saved, 2)
                os.close(saved)
                del os.environ["FLX_API_TIMING"]
            tmp.seek(0)
            stage_lines = tmp.read()
            m = re.search(rb"kmer long reads.*\((\d+) reads and (\d+) children of >= (\d+) bases, (\d+) words, (\d+) replayed\)", stage_lines)
            mc = re.search(rb"kmer long cover.*\((\d+) reads of >= (\d+) bases in (\d+) segments of (\d+) spans\)", stage_lines)
            if m:
                replayed = dict(long_reads=int(m.group(1)), long_children=int(m.group(2)), threshold=int(m.group(3)), words=int(m.group(4)),
                                words_replayed=int(m.group(5)))
        for _ in range(max(0, args.warmup - 1)):
            once()
        ts, parts = [], {"flx_score_kmer_cover": [], "flx_score_kmer_cover.long": [], "flx_score_kmer_fold": [], "flx_score_kmer_long": []}
        for _ in range(steps):
            ctx.timing_enable(True)
            ctx.timing_reset()
            t0 = time.perf_counter()
            once()
            ts.append((time.perf_counter() - t0) * 1e3)
            for k in parts:
                parts[k].append(ctx.timing_get(k)[0])
            ctx.timing_enable(False)
        nc = int(b["sc"].n_children)
        res = [b["t"][k].cpu().numpy().copy() for k in ("mean", "win", "pass")] + [b["t"]["crng"][:2 * nc].cpu().numpy().copy(),
                                                                                  b["t"]["cmean"][:nc].cpu().numpy().copy(), b["t"]["cwin"][:nc].cpu().numpy().copy()]
        row = {"row": name, "mode": "trim+split500" if children else "plain", "reads": b["n"], "bases": b["bases"], "FLX_KMER_LONG_MIN": long_min,
               "FLX_KMER_COVER_LONG_MIN": cover_min, "FLX_KMER_COVER_LONG_SPANS": spans, "ms_per_step": round(float(np.median(ts)), 3), "children": nc}
        for k, v in parts.items():
            row[k + "_ms"] = round(float(np.median(v)), 3)
        if replayed:
            row.update(replayed)
        if mc:
            row.update(cover_long_reads=int(mc.group(1)), cover_threshold=int(mc.group(2)), cover_segments=int(mc.group(3)), cover_spans=int(mc.group(4)))
        print(json.dumps(row), flush=True)
        rows.append(row)
        return row, res

    same = True

    def pair(name, b, children, steps=None):
        nonlocal same
        r_on, a = run(name, b, children, None, steps)
        r_cover_off, c0 = run(name, b, children, None, steps, cover_min=0)
        r_off, c = run(name, b, children, 0, steps, cover_min=0)
        for other in (c0, c):
            same = same and all(x.shape == y.shape and (x.view(np.uint8) == y.view(np.uint8)).all() for x, y in zip(a, other))
        return r_on, r_off, r_cover_off

    one = setup(np.zeros(0, dtype=np.int32), [long_read(4_000_000, 99)])
    one_plain = pair("one_4mbp_read", one, False)
    one_children = pair("one_4mbp_read", one, True)
    del one
    if args.crossover:
        for e in range(16, 23):
            b = setup(np.zeros(0, dtype=np.int32), [long_read(1 << e, 500 + e)])
            run("one_read_2^%d" % e, b, False, 1 << 12, 3, cover_min=1 << 12)  # (forced: the cooperative paths at every length)
            run("one_read_2^%d" % e, b, False, 0, 3, cover_min=0)
            del b
        b = setup(np.zeros(0, dtype=np.int32), [long_read(4_000_000, 99)])
        for spans in (8, 16, 32, 64, 128):
            run("one_4mbp_read_spans_%d" % spans, b, False, None, 3, spans=spans)
        del b
    if args.ultralong_only > 0:
        only = setup(np.random.default_rng(77).integers(100_000, 4_000_001, args.ultralong_only).astype(np.int32), [])
        pair("ultralong_only", only, False, 3)
        del only
        torch.cuda.empty_cache()
    if args.reads > 0:
        rng = np.random.default_rng(2024)
        extra = [long_read(int(L), 7000 + i) for i, L in enumerate(rng.integers(500_000, 4_000_001, args.extra))]
        withx = setup(synth.lengths(args.reads), extra)
        pair("c3_shape+%d_ultralong" % args.extra, withx, False)
        pair("c3_shape+%d_ultralong" % args.extra, withx, True)
        del withx
    for key in ("FLX_KMER_LONG_MIN", "FLX_KMER_COVER_LONG_MIN", "FLX_KMER_COVER_LONG_SPANS"):
        os.environ.pop(key, None)
    summary = {"summary": "ultra-long reads, k-mer mode, window %d" % args.window_size, "device": ctx.device_info()["name"],
               "one_4mbp_cover_ms": one_plain[0]["flx_score_kmer_cover_ms"], "one_4mbp_cover_one_wave_ms": one_plain[2]["flx_score_kmer_cover_ms"],
               "one_4mbp_long_ms": one_plain[0]["flx_score_kmer_long_ms"], "one_4mbp_one_lane_fold_ms": one_plain[1]["flx_score_kmer_fold_ms"],
               "one_4mbp_children_long_ms": one_children[0]["flx_score_kmer_long_ms"],
               "one_4mbp_children_one_lane_fold_ms": one_children[1]["flx_score_kmer_fold_ms"],
               "same_bits_with_and_without_the_path": bool(same)}
    print(json.dumps(summary), flush=True)
    if args.out:
        with open(args.out, "a") as fh:
            for r in rows + [summary]:
                fh.write(json.dumps(r) + "\n")
    ks.close()
    ctx.close()
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
