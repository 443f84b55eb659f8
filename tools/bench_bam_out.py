#!/usr/bin/env python3
"""--bam: the device-resident rate of the encode kernels alone (flx_bam_from_fastq_dev, GB/s of text in, against the bytes they must
move: ~2 B in and ~1.5 B out per base at the 8 TB/s of the HBM), the host-to-host rate of flx_bgzf_bam_from_fastq beside
flx_bgzf_compress on the same text, and the wall time of the whole command line (`filtlong --keep_percent 90`) with --bam, with
--gzip and plain — one warm-up run each, then --steps timed runs each, alternating, stdout to /dev/null; medians with min and max,
and the `output` stage of FLX_CLI_TIMING for each.  One JSON line, appended to profiles/bam_out.jsonl (--out).  The input is the
ONT-like FASTQ of tools/gen_fastq_ont.py, written to --dir.

    python3 tools/bench_bam_out.py --bytes 2147483648 --steps 5 --dir /tmp/bench_bam_out
"""
import argparse
import json
import os
import re
import subprocess
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
HBM_PEAK_GBPS = 8000.0  # MI355X


def spread(times):
    t = sorted(times)
    return {"median_s": t[len(t) // 2], "min_s": t[0], "max_s": t[-1]}


def record_offsets(text):
    """four-line FASTQ: a record ends behind every fourth newline"""
    nl = np.flatnonzero(np.frombuffer(text, dtype=np.uint8) == 10)
    assert len(nl) % 4 == 0
    return np.concatenate(([0], nl[3::4] + 1)).astype(np.uint64)


def device_rate(ctx, torch, text, rec_off, steps, warmup):
    from filtlong_amd import api
    n = len(rec_off) - 1
    cap = api.bam_from_fastq_bound(len(text), n)
    d_in = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).to("cuda")
    d_ro = torch.from_numpy(rec_off.view(np.int64).copy()).to("cuda")
    d_out = torch.empty(cap + 16, dtype=torch.uint8, device="cuda")
    d_oo = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    call = lambda: ctx.bam_from_fastq_dev(d_in.data_ptr(), len(text), d_ro.data_ptr(), n, d_out.data_ptr(), cap, d_oo.data_ptr())
    for _ in range(warmup):
        out_len, bad = call()
        assert bad == n
    times = []
    ctx.timing_enable(True)
    for _ in range(steps):
        ctx.timing_reset()
        out_len, bad = call()
        times.append(ctx.timing_get("flx_bam_encode")[0] / 1e3)
    ctx.timing_enable(False)
    r = spread(times)
    moved = len(text) + out_len
    r.update(records=n, text_bytes=len(text), bam_bytes=out_len, gbps_text_in_median=len(text) / r["median_s"] / 1e9,
             gbps_algorithmic_median=moved / r["median_s"] / 1e9, fraction_of_hbm_roofline=moved / r["median_s"] / 1e9 / HBM_PEAK_GBPS)
    return r


def host_rate(ctx, text, rec_off, steps, threads=16, piece=16 << 20):
    """pieces of ~16 MiB of whole records from `threads` threads at once, as the command line's workers call it"""
    from filtlong_amd import api
    cuts = [0]
    for k in range(1, len(rec_off)):
        if int(rec_off[k]) - int(rec_off[cuts[-1]]) >= piece or k == len(rec_off) - 1:
            cuts.append(k)
    pieces = [(text[int(rec_off[a]):int(rec_off[b])], rec_off[a:b + 1] - rec_off[a]) for a, b in zip(cuts, cuts[1:])]
    out = {}
    for what in ("bam_from_fastq", "compress"):
        z = api.Bgzf(ctx, slot_bytes=20 << 20, slots=threads)
        times, sizes = [], [0] * len(pieces)

        def work(t):
            for j in range(t, len(pieces), threads):
                p, off = pieces[j]
                sizes[j] = len(api.bgzf_bam_from_fastq(z, p, off, eof=False) if what == "bam_from_fastq" else z.compress(p, eof=False))
        for _ in range(steps + 1):  # (the first run warms up and lets the slots grow)
            t0 = time.perf_counter()
            th = [threading.Thread(target=work, args=(t,)) for t in range(threads)]
            for x in th:
                x.start()
            for x in th:
                x.join()
            times.append(time.perf_counter() - t0)
        z.close()
        r = spread(times[1:])
        r.update(pieces=len(pieces), compressed_bytes=sum(sizes), gbps_text_median=len(text) / r["median_s"] / 1e9,
                 note="includes the Python wrapper's copies of every piece")
        out[what] = r
    return out


def cli_times(fastq_path, steps):
    exe = os.path.join(ROOT, "filtlong_amd", "bin", "filtlong")
    settings = {"bam": ["--bam"], "gzip": ["--gzip"], "plain": []}
    times = {k: [] for k in settings}
    stage = {k: [] for k in settings}
    for step in range(steps + 1):  # one warm-up run each, then alternating: every setting sees the same machine
        for k, flags in settings.items():
            t0 = time.perf_counter()
            p = subprocess.run([exe] + flags + ["--keep_percent", "90", fastq_path], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE,
                               env=dict(os.environ, FLX_CLI_TIMING="1"))
            t = time.perf_counter() - t0
            if p.returncode != 0:
                raise RuntimeError("%s: exit %d: %s" % (k, p.returncode, p.stderr.decode(errors="replace")[-400:]))
            if step > 0:
                times[k].append(t)
                m = re.search(r"\[timing\] output\s+([0-9.]+) s", p.stderr.decode(errors="replace"))
                if m:
                    stage[k].append(float(m.group(1)))
    out = {k: spread(v) for k, v in times.items()}
    for k in settings:
        out[k]["output_stage_s"] = sorted(stage[k])
        out[k]["note"] = "FLX_CLI_TIMING=1 is set: the context is created in line and torn down at the end, in all three alike"
    out["bam_not_slower_than_gzip"] = out["bam"]["median_s"] <= out["gzip"]["median_s"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=int, default=2 << 30, help="bytes of FASTQ")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--dir", default="/tmp/bench_bam_out", help="where the FASTQ is written")
    ap.add_argument("--no-cli", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bam_out.jsonl"))
    a = ap.parse_args()
    import torch
    import gen_fastq_ont
    from filtlong_amd import api
    os.makedirs(a.dir, exist_ok=True)
    t0 = time.perf_counter()
    fastq = gen_fastq_ont.generate(a.bytes, seed=1)
    fastq_path = os.path.join(a.dir, "ont.fastq")
    with open(fastq_path, "wb") as f:
        f.write(fastq)
    rec_off = record_offsets(fastq)
    print("input: %d bytes of FASTQ, %d records, %.1f s" % (len(fastq), len(rec_off) - 1, time.perf_counter() - t0), file=sys.stderr, flush=True)
    ctx = api.Context(0)
    res = {"tool": "bench_bam_out", "device": ctx.device_info()["name"], "time": time.strftime("%Y-%m-%dT%H:%M:%SZ", time.gmtime()),
           "fastq_bytes": len(fastq)}
    res["device_resident"] = device_rate(ctx, torch, fastq, rec_off, a.steps, a.warmup)
    print(json.dumps(res["device_resident"], sort_keys=True), file=sys.stderr, flush=True)
    res["host_to_host"] = host_rate(ctx, fastq, rec_off, a.steps)
    print(json.dumps(res["host_to_host"], sort_keys=True), file=sys.stderr, flush=True)
    ctx.close()
    del fastq
    if not a.no_cli:
        res["cli"] = cli_times(fastq_path, a.steps)
    line = json.dumps(res, sort_keys=True)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
