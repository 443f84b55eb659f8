#!/usr/bin/env python3
"""Time the adapter detection alone (flx_adapter_cuts_dev, its bracket "flx_adapters") with and without --adapter_overhang, over N
reads resident in HBM, for sets of 4 and 256 patterns (random sequences of 28 bases), W = 150, E = 20:
  O = 0 and O = 8 on the build of this tree, and, with --parent-lib, O = 0 on a build of the parent commit (its libfiltlong_hip.so).
Every library runs in a fresh child process of its own (the library is chosen when it is loaded); the children ALTERNATE, tree, parent,
tree, parent ..., --rounds times, so that the spread between rounds of the SAME code is measured beside the difference between the two.
Per (patterns, O): the median of --steps calls behind a warm-up in every round; `spread_ms` is the largest minus the smallest of the
rounds' medians of one code, `tree_minus_parent_ms` the difference of the medians over all rounds.  10 % of the reads begin inside an
adapter (6 to 8 of its bases missing); the keys' checksum shows that both libraries computed the same at O = 0.
Lengths follow the benchmark's C2 configuration (filtlong_amd.synth.lengths).  One JSON line on stdout, appended to --out
(profiles/adapters_overhang.jsonl) when given."""
import argparse
import json
import os
import subprocess
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def worker(args):
    import ctypes as C
    import torch
    from filtlong_amd import api, synth
    ctx = api.Context(0)
    n = args.reads
    lengths = synth.lengths(n).astype(np.int32)
    offsets = np.zeros(n, dtype=np.uint64)
    pb = C.c_uint64()
    assert ctx.L.flx_plane_layout(lengths.ctypes.data, n, offsets.ctypes.data, C.byref(pb)) == 0
    order = api.length_order(lengths)
    d_len, d_ord = torch.from_numpy(lengths).cuda(), torch.from_numpy(order.astype(np.int32)).cuda()
    d_off = torch.from_numpy(offsets.astype(np.int64)).cuda()
    d_keys = torch.empty(2 * n, dtype=torch.int32, device="cuda")
    gen = torch.Generator(device="cuda").manual_seed(3)
    acgt = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device="cuda")
    d_base = acgt[torch.randint(0, 4, (pb.value,), generator=gen, device="cuda")]
    ctx.timing_enable(True)
    out = {"library": os.environ.get("FLX_LIB_PATH", "tree"), "device": ctx.device_info()["name"], "bases": int(lengths.astype(np.int64).sum())}
    for n_pat in [int(v) for v in args.patterns.split(",")]:
        srng = np.random.default_rng(n_pat)
        seqs = [np.frombuffer(b"ACGT", dtype=np.uint8)[srng.integers(0, 4, size=28)].tobytes() for _ in range(n_pat // 2)]
        d_seq = d_base.clone()
        prng = np.random.default_rng(11)
        drawn = np.flatnonzero((prng.random(n) < 0.1) & (lengths > 200))
        at, what = [], []
        for i in drawn:  # the read begins inside an adapter
            s = seqs[int(prng.integers(0, len(seqs)))][int(prng.integers(6, 9)):]
            at.append(np.arange(len(s), dtype=np.int64) + int(offsets[i]))
            what.append(np.frombuffer(s, dtype=np.uint8))
        if at:
            d_seq[torch.from_numpy(np.concatenate(at)).cuda()] = torch.from_numpy(np.concatenate(what)).cuda()
        for overhang in [int(v) for v in args.overhangs.split(",")]:
            ad = api.Adapters(seqs, errors=20, window=150, overhang=overhang)
            ms = []
            for step in range(args.steps + 2):  # (the first two are the warm-up)
                ctx.timing_reset()
                ctx.adapter_cuts_dev(ad, d_seq.data_ptr(), d_seq.numel(), d_off.data_ptr(), d_len.data_ptr(), d_ord.data_ptr(), n, d_keys.data_ptr())
                ctx.synchronize()
                if step >= 2:
                    ms.append(ctx.timing_get("flx_adapters")[0])
            keys = d_keys.cpu().numpy().astype(np.uint32)
            out["p_%d_o_%d" % (n_pat, overhang)] = {"median_ms": round(float(np.median(ms)), 4), "best_ms": round(min(ms), 4), "worst_ms": round(max(ms), 4),
                                                    "hits": int((keys > 0).sum()), "keys_crc32": zlib.crc32(keys.tobytes())}
            ad.close()
        del d_seq
    ctx.close()
    print("WORKER " + json.dumps(out, sort_keys=True))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=100_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--patterns", default="4,256")
    ap.add_argument("--overhangs", default="0,8")
    ap.add_argument("--parent-lib", default=None, help="libfiltlong_hip.so of the parent commit: O = 0 is measured on it as well")
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=None)
    ap.add_argument("--worker", action="store_true")
    args = ap.parse_args()
    if args.worker:
        return worker(args)

    def child(lib, overhangs):
        env = dict(os.environ)
        env.pop("FLX_LIB_PATH", None)
        if lib:
            env["FLX_LIB_PATH"] = lib
        cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--reads", str(args.reads), "--steps", str(args.steps), "--patterns", args.patterns,
               "--overhangs", overhangs]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=600)
        if p.returncode != 0:
            raise SystemExit("worker failed (%d): %s" % (p.returncode, p.stderr.decode()[-2000:]))
        return json.loads([ln for ln in p.stdout.decode().splitlines() if ln.startswith("WORKER ")][-1][7:])

    rounds = []
    for _ in range(args.rounds):
        rounds.append({"tree": child(None, args.overhangs), "parent": child(args.parent_lib, "0") if args.parent_lib else None})
    rec = {"tool": "bench_adapters_overhang", "label": args.label, "time": time.strftime("%Y-%m-%dT%H:%M:%SZ", time.gmtime()),
           "device": rounds[0]["tree"]["device"], "reads": args.reads, "bases": rounds[0]["tree"]["bases"], "steps": args.steps, "rounds": args.rounds,
           "window": 150, "errors": 20}
    for n_pat in [int(v) for v in args.patterns.split(",")]:
        m = {}
        for overhang in [int(v) for v in args.overhangs.split(",")]:
            k = "p_%d_o_%d" % (n_pat, overhang)
            meds = [r["tree"][k]["median_ms"] for r in rounds]
            m["tree_o_%d" % overhang] = {"round_medians_ms": meds, "median_ms": round(float(np.median(meds)), 4), "spread_ms": round(max(meds) - min(meds), 4),
                                         "hits": rounds[0]["tree"][k]["hits"], "keys_crc32": rounds[0]["tree"][k]["keys_crc32"]}
        if "tree_o_0" in m:
            for overhang in [int(v) for v in args.overhangs.split(",") if int(v)]:
                m["o_%d_over_o_0" % overhang] = round(m["tree_o_%d" % overhang]["median_ms"] / m["tree_o_0"]["median_ms"], 3)
        if args.parent_lib and "tree_o_0" in m:
            k = "p_%d_o_0" % n_pat
            meds = [r["parent"][k]["median_ms"] for r in rounds]
            m["parent_o_0"] = {"round_medians_ms": meds, "median_ms": round(float(np.median(meds)), 4), "spread_ms": round(max(meds) - min(meds), 4),
                               "hits": rounds[0]["parent"][k]["hits"], "keys_crc32": rounds[0]["parent"][k]["keys_crc32"]}
            m["tree_minus_parent_ms"] = round(m["tree_o_0"]["median_ms"] - m["parent_o_0"]["median_ms"], 4)
            m["same_keys_as_parent"] = m["tree_o_0"]["keys_crc32"] == m["parent_o_0"]["keys_crc32"]
        rec["p_%d" % n_pat] = m
    line = json.dumps(rec, sort_keys=True)
    print(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
