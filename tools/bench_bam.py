#!/usr/bin/env python3
"""Unaligned BAM to FASTQ text: the device-resident rate of flx_bam_to_fastq_dev against the HBM roofline (algorithmic bytes =
inflated BAM + text), the host-to-host rate of flx_bam_to_fastq, and the whole command line (`filtlong --keep_percent 90`) on the BAM
with FLX_CLI_GPU_BAM at 1 and at 0 and on the FASTQ the BAM was made from — one warm-up run each, then --steps timed runs each,
alternating; medians with min and max.  One JSON line, appended to profiles/bam.jsonl (--out).  The input is the ONT-like FASTQ of
tools/gen_fastq_ont.py through tools/gen_bam.py, written to --dir.

    python3 tools/bench_bam.py --bytes 2147483648 --steps 5 --dir /tmp/bench_bam
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
HBM_PEAK_GBPS = 8000.0  # MI355X


def spread(times):
    t = sorted(times)
    return {"median_s": t[len(t) // 2], "min_s": t[0], "max_s": t[-1]}


def device_rate(ctx, torch, bam, steps, warmup):
    from filtlong_amd import api
    rec_off, end = api.bam_index(bam)
    assert end == api.BAM_END
    n = len(rec_off) - 1
    cap = 2 * int(rec_off[n] - rec_off[0])
    d_in = torch.from_numpy(np.frombuffer(bam, dtype=np.uint8).copy()).to("cuda")
    d_ro = torch.from_numpy(rec_off.view(np.int64)).to("cuda")
    d_out = torch.empty(cap, dtype=torch.uint8, device="cuda")
    d_oo = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    call = lambda: ctx.bam_to_fastq_dev(d_in.data_ptr(), len(bam), d_ro.data_ptr(), n, d_out.data_ptr(), cap, d_oo.data_ptr())
    for _ in range(warmup):
        out_len, skipped, bad = call()
        assert bad == n
    times = []
    ctx.timing_enable(True)
    for _ in range(steps):
        ctx.timing_reset()
        out_len, skipped, bad = call()
        times.append(ctx.timing_get("flx_bam")[0] / 1e3)
    ctx.timing_enable(False)
    r = spread(times)
    moved = len(bam) + out_len
    r.update(records=n, bam_bytes=len(bam), text_bytes=out_len, gbps_algorithmic_median=moved / r["median_s"] / 1e9,
             fraction_of_hbm_roofline=moved / r["median_s"] / 1e9 / HBM_PEAK_GBPS)
    return r


def host_rate(ctx, bam, steps):
    from filtlong_amd import api
    times = []
    for _ in range(steps + 1):  # (the first run warms up)
        t0 = time.perf_counter()
        text = api.bam_to_fastq(ctx, bam)
        times.append(time.perf_counter() - t0)
    r = spread(times[1:])
    r.update(bam_bytes=len(bam), text_bytes=len(text), gbps_text_median=len(text) / r["median_s"] / 1e9,
             note="includes the Python wrapper's index walk and buffer allocation")
    return r


def cli_times(bam_path, fastq_path, steps):
    exe = os.path.join(ROOT, "filtlong_amd", "bin", "filtlong")
    settings = {"bam_switch_1": (bam_path, {"FLX_CLI_GPU_BAM": "1"}), "bam_switch_0": (bam_path, {"FLX_CLI_GPU_BAM": "0"}),
                "fastq": (fastq_path, {})}
    times = {k: [] for k in settings}
    lines = {}
    for step in range(steps + 1):  # one warm-up run each, then alternating: every setting sees the same machine
        for k, (path, env) in settings.items():
            t0 = time.perf_counter()
            p = subprocess.run([exe, "--keep_percent", "90", path], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE,
                               env=dict(os.environ, FLX_CLI_BAM_TIMING="1", **env))
            t = time.perf_counter() - t0
            if p.returncode != 0:
                raise RuntimeError("%s: exit %d: %s" % (k, p.returncode, p.stderr.decode(errors="replace")[-400:]))
            if step > 0:
                times[k].append(t)
                lines.setdefault(k, []).extend(l for l in p.stderr.decode(errors="replace").splitlines() if l.startswith("[bam]"))
    out = {k: spread(v) for k, v in times.items()}
    for k in ("bam_switch_1", "bam_switch_0"):
        out[k]["transcode_ms"] = sorted(float(l.split(",")[-1].split()[0]) for l in lines[k])
        out[k]["path"] = sorted(set(l.split(",")[-2].strip() for l in lines[k]))
    out["default_by_the_rule"] = 1 if out["bam_switch_1"]["median_s"] < out["bam_switch_0"]["min_s"] else 0
    out.update(bam_file_bytes=os.path.getsize(bam_path), fastq_file_bytes=os.path.getsize(fastq_path))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=int, default=2 << 30, help="bytes of FASTQ")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--dir", default="/tmp/bench_bam", help="where the FASTQ and the BAM are written")
    ap.add_argument("--no-cli", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bam.jsonl"))
    a = ap.parse_args()
    import torch
    import gen_bam
    import gen_fastq_ont
    from filtlong_amd import api
    os.makedirs(a.dir, exist_ok=True)
    t0 = time.perf_counter()
    fastq = gen_fastq_ont.generate(a.bytes, seed=1)  # (generated whole: a repeated block would repeat its read names)
    bam = gen_bam.fastq_to_bam(fastq)
    fastq_path, bam_path = os.path.join(a.dir, "ont.fastq"), os.path.join(a.dir, "ont.bam")
    with open(fastq_path, "wb") as f:
        f.write(fastq)
    with open(bam_path, "wb") as f:
        f.write(gen_bam.bgzf(bam, 1, 16))
    n_fastq = len(fastq)
    del fastq
    print("inputs: %d bytes of FASTQ, %d of BAM, %.1f s" % (n_fastq, len(bam), time.perf_counter() - t0), file=sys.stderr, flush=True)
    ctx = api.Context(0)
    res = {"tool": "bench_bam", "device": ctx.device_info()["name"], "time": time.strftime("%Y-%m-%dT%H:%M:%SZ", time.gmtime()),
           "fastq_bytes": n_fastq}
    res["device_resident"] = device_rate(ctx, torch, bam, a.steps, a.warmup)
    print(json.dumps(res["device_resident"], sort_keys=True), file=sys.stderr, flush=True)
    res["host_to_host"] = host_rate(ctx, bam, a.steps)
    print(json.dumps(res["host_to_host"], sort_keys=True), file=sys.stderr, flush=True)
    ctx.close()
    del bam
    if not a.no_cli:
        res["cli"] = cli_times(bam_path, fastq_path, a.steps)
    line = json.dumps(res, sort_keys=True)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
