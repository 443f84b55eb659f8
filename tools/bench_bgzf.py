#!/usr/bin/env python3
"""BGZF compression on the GPU: device-resident throughput of flx_bgzf_compress_dev on an ONT-like FASTQ
(tools/gen_fastq_ont.py) and on random bytes, the compressed sizes against zlib levels 1 and 6 on the same 65280-byte grid,
and (--cli FILE) the command line's wall time plain against --gzip and against `plain | gzip -1`.  One JSON line per run,
appended to profiles/bgzf.jsonl (--out).  Kernel times: run it under `rocprofv3 --kernel-trace --stats -- python3 ...`.

    python3 tools/bench_bgzf.py --bytes 1073741824 --steps 5

--inflate measures the read side instead (one JSON line, profiles/bgzf_inflate.jsonl): the device-resident rate of
flx_bgzf_inflate_dev (output bytes per second) on the ONT-like FASTQ as BGZF from zlib -1, zlib -6 and this repository's encoder,
the host-to-host rate of flx_bgzf_inflate from 1 / 4 / 16 threads, and (--cli FILE, a BGZF FASTQ) the command line's wall time
with FLX_CLI_GPU_INFLATE at 0, at 1 and at 1 with FLX_CLI_GPU_INFLATE_OUTPUT=1, alternating; medians with the spread (min, max) beside them.
"""
import argparse
import json
import os
import shutil
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def device_rate(ctx, torch, data, steps, warmup):
    from filtlong_amd import api
    d_in = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to("cuda")
    cap = api.bgzf_bound(len(data))
    d_out = torch.empty(cap, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for _ in range(warmup):
        ctx.bgzf_compress_dev(d_in.data_ptr(), len(data), d_out.data_ptr(), cap)
    times = []
    ctx.timing_enable(True)
    for _ in range(steps):
        ctx.timing_reset()
        t0 = time.perf_counter()
        got = ctx.bgzf_compress_dev(d_in.data_ptr(), len(data), d_out.data_ptr(), cap)
        wall = time.perf_counter() - t0
        ms, _ = ctx.timing_get("flx_bgzf")
        times.append((wall, ms / 1e3))
    ctx.timing_enable(False)
    best_wall = min(t[0] for t in times)
    best_dev = min(t[1] for t in times)
    med_dev = sorted(t[1] for t in times)[len(times) // 2]
    return {"bytes": len(data), "compressed": got, "ratio": got / len(data), "wall_s_best": best_wall,
            "device_s_best": best_dev, "device_s_median": med_dev, "gbps_device_best": len(data) / best_dev / 1e9,
            "gbps_device_median": len(data) / med_dev / 1e9, "gbps_wall_best": len(data) / best_wall / 1e9}


def cli_times(path, steps):
    exe = os.path.join(ROOT, "filtlong_amd", "bin", "filtlong")
    args = [exe, "--keep_percent", "90", path]
    out = {}
    for name, extra in (("plain", []), ("gzip", ["--gzip"])):
        best = None
        for _ in range(steps):
            t0 = time.perf_counter()
            with open(os.devnull, "wb") as null:
                subprocess.run(args[:1] + extra + args[1:], stdout=null, stderr=subprocess.DEVNULL, check=True)
            t = time.perf_counter() - t0
            best = t if best is None else min(best, t)
        out[name + "_s"] = best
    if shutil.which("gzip"):
        t0 = time.perf_counter()
        subprocess.run("%s --keep_percent 90 %s 2>/dev/null | gzip -1 > /dev/null" % (exe, path), shell=True, check=True)
        out["plain_pipe_gzip1_s"] = time.perf_counter() - t0
    return out


def spread(times):
    t = sorted(times)
    return {"median_s": t[len(t) // 2], "min_s": t[0], "max_s": t[-1]}


def inflate_device_rate(ctx, torch, stream, steps, warmup):
    from filtlong_amd import api
    in_off, out_off = api.bgzf_index(stream)
    n, total = len(in_off) - 1, int(out_off[-1])
    d_in = torch.from_numpy(np.frombuffer(stream, dtype=np.uint8).copy()).to("cuda")
    d_io = torch.from_numpy(in_off.view(np.int64)).to("cuda")
    d_oo = torch.from_numpy(out_off.view(np.int64)).to("cuda")
    d_out = torch.empty(total, dtype=torch.uint8, device="cuda")
    d_st = torch.empty(n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    call = lambda: ctx.bgzf_inflate_dev(d_in.data_ptr(), d_io.data_ptr(), d_oo.data_ptr(), n, d_out.data_ptr(), d_st.data_ptr())
    for _ in range(warmup):
        assert call() == n
    times = []
    ctx.timing_enable(True)
    for _ in range(steps):
        ctx.timing_reset()
        assert call() == n
        times.append(ctx.timing_get("flx_bgzf_inflate")[0] / 1e3)
    ctx.timing_enable(False)
    r = spread(times)
    r.update(members=n, compressed=len(stream), bytes=total, gbps_out_median=total / r["median_s"] / 1e9)
    return r


def inflate_host_rate(z, stream, threads, steps):
    import threading
    from filtlong_amd import api
    in_off, out_off = api.bgzf_index(stream)
    n = len(in_off) - 1
    cuts = [n * k // threads for k in range(threads + 1)]
    parts = [stream[int(in_off[cuts[k]]):int(in_off[cuts[k + 1]])] for k in range(threads)]
    total = int(out_off[-1])
    times = []
    for _ in range(steps + 1):  # (the first run warms the slots up)
        th = [threading.Thread(target=z.inflate, args=(p,)) for p in parts]
        t0 = time.perf_counter()
        for t in th:
            t.start()
        for t in th:
            t.join()
        times.append(time.perf_counter() - t0)
    r = spread(times[1:])
    r.update(threads=threads, bytes=total, gbps_out_median=total / r["median_s"] / 1e9)
    return r


def inflate_cli_times(path, steps):
    exe = os.path.join(ROOT, "filtlong_amd", "bin", "filtlong")
    settings = {"switch_0": {"FLX_CLI_GPU_INFLATE": "0"}, "switch_1": {"FLX_CLI_GPU_INFLATE": "1"},
                "switch_1_output_pass": {"FLX_CLI_GPU_INFLATE": "1", "FLX_CLI_GPU_INFLATE_OUTPUT": "1"}}
    times = {k: [] for k in settings}
    for _ in range(steps):
        for k, env in settings.items():  # alternating: every setting sees the same machine
            t0 = time.perf_counter()
            p = subprocess.run([exe, "--keep_percent", "90", path], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE,
                               env=dict(os.environ, **env))
            if p.returncode != 0:
                raise RuntimeError("%s: exit %d: %s" % (k, p.returncode, p.stderr.decode(errors="replace")[-400:]))
            times[k].append(time.perf_counter() - t0)
    return dict({k: spread(v) for k, v in times.items()}, file_bytes=os.path.getsize(path))


def inflate_main(a):
    import torch
    import _bgzf
    import gen_fastq_ont
    from filtlong_amd import api
    block = gen_fastq_ont.generate(min(a.bytes, 256 << 20), seed=1)
    ont = (block * (a.bytes // len(block) + 1))[:a.bytes]
    ctx = api.Context(0)
    res = {"tool": "bench_bgzf --inflate", "device": ctx.device_info()["name"], "time": time.strftime("%Y-%m-%dT%H:%M:%SZ", time.gmtime())}
    z = api.Bgzf(ctx, slot_bytes=16 << 20, slots=16)
    streams = {"zlib1": _bgzf.zlib_bgzf(ont, 1), "zlib6": _bgzf.zlib_bgzf(ont, 6), "own": z.compress(ont)}
    res["device"] = {k: inflate_device_rate(ctx, torch, s, a.steps, a.warmup) for k, s in streams.items()}
    print(json.dumps(res["device"], sort_keys=True), file=sys.stderr, flush=True)  # (a long run: every part as soon as it is there)
    res["host_to_host"] = [inflate_host_rate(z, streams["zlib6"], t, a.steps) for t in (1, 4, 16)]
    print(json.dumps(res["host_to_host"], sort_keys=True), file=sys.stderr, flush=True)
    z.close()
    ctx.close()
    if a.cli:
        res["cli"] = inflate_cli_times(a.cli, a.steps)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=int, default=1 << 30)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--zlib-sample", type=int, default=64 << 20, help="bytes compressed by zlib for the size comparison")
    ap.add_argument("--cli", default=None, help="a FASTQ for the command-line timings")
    ap.add_argument("--inflate", action="store_true", help="measure the inflater (see above)")
    ap.add_argument("--out", default=None, help="default profiles/bgzf.jsonl, with --inflate profiles/bgzf_inflate.jsonl")
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "bgzf_inflate.jsonl" if a.inflate else "bgzf.jsonl")
    if a.inflate:
        line = json.dumps(inflate_main(a), sort_keys=True)
        print(line)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")
        return
    import torch
    import _bgzf
    import gen_fastq_ont
    from filtlong_amd import api

    block = gen_fastq_ont.generate(min(a.bytes, 256 << 20), seed=1)
    ont = (block * (a.bytes // len(block) + 1))[:a.bytes]
    rnd = np.random.default_rng(1).integers(0, 256, a.bytes, dtype=np.uint8).tobytes()
    ctx = api.Context(0)
    res = {"tool": "bench_bgzf", "device": ctx.device_info()["name"], "time": time.strftime("%Y-%m-%dT%H:%M:%SZ", time.gmtime())}
    res["ont"] = device_rate(ctx, torch, ont, a.steps, a.warmup)
    res["random"] = device_rate(ctx, torch, rnd, a.steps, a.warmup)
    sample = block[:a.zlib_sample]
    d_in = torch.from_numpy(np.frombuffer(sample, dtype=np.uint8).copy()).to("cuda")
    d_out = torch.empty(api.bgzf_bound(len(sample)), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    gpu = ctx.bgzf_compress_dev(d_in.data_ptr(), len(sample), d_out.data_ptr(), api.bgzf_bound(len(sample)))
    res["sizes"] = {"bytes": len(sample), "gpu": gpu, "zlib1": len(_bgzf.zlib_bgzf(sample, 1)), "zlib6": len(_bgzf.zlib_bgzf(sample, 6))}
    res["sizes"]["gpu_over_zlib1"] = gpu / res["sizes"]["zlib1"]
    res["sizes"]["gpu_over_zlib6"] = gpu / res["sizes"]["zlib6"]
    ctx.close()
    if a.cli:
        res["cli"] = dict(cli_times(a.cli, a.steps), file_bytes=os.path.getsize(a.cli))
    line = json.dumps(res, sort_keys=True)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
