#!/usr/bin/env python3
"""Seeded ONT-like FASTQ: random bases, qualities with a slowly varying mean plus noise, ONT-style headers
(`@uuid runid=... read=... ch=... start_time=...`).  Unlike tools/gen_fastq.cpp (a repeated "ACGT" sequence) it compresses
about like real nanopore output, which is what the BGZF measurements need.

    python3 tools/gen_fastq_ont.py OUT.fastq --bytes 1073741824 --seed 1
"""
import argparse
import sys

import numpy as np

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def records(rng, runid):
    read = 0
    t = 1_700_000_000
    while True:
        n = int(min(max(rng.lognormal(8.6, 0.9), 200), 120_000))
        seq = ACGT[rng.integers(0, 4, n)]
        # mean quality: a random walk with a slow drift over the read, per-base noise on top
        steps = max(n // 500, 1)
        walk = np.cumsum(rng.normal(0.0, 0.8, steps + 1)) + rng.uniform(8, 20)
        mean = np.interp(np.arange(n), np.linspace(0, n - 1, steps + 1), walk)
        q = np.clip(np.rint(mean + rng.normal(0.0, 3.5, n)), 1, 50).astype(np.uint8) + 33
        uuid = rng.integers(0, 16, 32)
        u = "".join("0123456789abcdef"[x] for x in uuid)
        u = "%s-%s-%s-%s-%s" % (u[:8], u[8:12], u[12:16], u[16:20], u[20:])
        t += int(rng.integers(0, 30))
        hdr = "@%s runid=%s read=%d ch=%d start_time=%s\n" % (
            u, runid, read, int(rng.integers(1, 513)),
            np.datetime_as_string(np.datetime64(t, "s")) + "Z")
        read += 1
        yield hdr.encode() + seq.tobytes() + b"\n+\n" + q.tobytes() + b"\n"


def generate(size, seed=1):
    """At least `size` bytes of whole records."""
    rng = np.random.default_rng(seed)
    runid = "".join("0123456789abcdef"[x] for x in rng.integers(0, 16, 40))
    out, total = [], 0
    for r in records(rng, runid):
        out.append(r)
        total += len(r)
        if total >= size:
            break
    return b"".join(out)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("out")
    ap.add_argument("--bytes", type=int, default=1 << 30)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args(argv)
    rng = np.random.default_rng(a.seed)
    runid = "".join("0123456789abcdef"[x] for x in rng.integers(0, 16, 40))
    total = 0
    with open(a.out, "wb") as f:
        for r in records(rng, runid):
            f.write(r)
            total += len(r)
            if total >= a.bytes:
                break
    print("%s: %d bytes" % (a.out, total), file=sys.stderr)


if __name__ == "__main__":
    main()
