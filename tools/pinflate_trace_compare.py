#!/usr/bin/env python3
"""Two builds of the command line's gzip reader, one trace each, compared line by line.

    tools/pinflate_trace_compare.py OTHER_TREE [WORKDIR]

Compiles tests/pinflate_layers_host.cpp twice: against this tree's filtlong_amd/{cli,csrc} and against OTHER_TREE's (a checkout or
`git archive` of the commit to compare with).  Both programs read the corpus of tests/test_cli_pinflate.py and
tests/test_pinflate_device_host.py (compression levels, the odd streams, BGZF alone and mixed with plain members, the truncated,
bit-flipped, CRC and ISIZE cases) at chunk sizes 700 / 4096 / 65536 with 2 / 5 / 16 threads, with and without the device stub.
What is compared: the program's whole output (bytes, access points, end state, counters, the device stub's calls) and the reader's
own FLX_CLI_PINFLATE_TIMING lines with the times taken out (rounds, chunks chained, bytes by zlib, members handed to zlib).
Prints the number of cases compared and every case that differs; exit status 1 if any does.  Two kinds of case are set apart: files
named fixed_* (a damaged BGZF header that the reader before the layers took two ways: expected to differ), and cases whose trace
depends on timing in both builds (each build is then run many times at once, and both must give the same set of traces)."""
import concurrent.futures
import gzip
import os
import re
import struct
import subprocess
import sys
import tempfile
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import _bgzf  # noqa: E402
import _cases  # noqa: E402
import test_cli_pinflate as T  # noqa: E402  (the generators only)


def corpus():
    c = {}
    rng = np.random.RandomState(20250925)
    data = T.read_like_fastq(rng, 600, 5000)
    for level in (1, 2, 4, 6, 9):
        c["level%d" % level] = T.gz_with_name(data, level) if level % 2 == 0 else gzip.compress(data, level, mtime=0)
    rng = np.random.RandomState(3)
    genome = bytes(rng.choice(list(b"ACGT"), size=3000000).astype(np.uint8))
    c["sparse"] = gzip.compress(T.read_like_fastq(rng, 500, 6000, genome=genome), 6, mtime=0)
    c["periodic"] = gzip.compress(T.read_like_fastq(np.random.RandomState(7), 300, 5000, periodic=True), 6, mtime=0)

    rng = np.random.RandomState(11)
    data = T.read_like_fastq(rng, 150, 3000)

    def deflate(d, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
        z = zlib.compressobj(level, zlib.DEFLATED, 31, 9, strategy)
        return z.compress(d) + z.flush()

    def flushed(d, every, how):
        z = zlib.compressobj(6, zlib.DEFLATED, 31)
        out = b""
        for a in range(0, len(d), every):
            out += z.compress(d[a:a + every]) + z.flush(how)
        return out + z.flush()

    cuts = [0, 100000, 100001, len(data) // 2, len(data)]
    c.update({
        "odd_stored": gzip.compress(data, 0, mtime=0),
        "odd_fixed": deflate(data, strategy=zlib.Z_FIXED),
        "odd_huffman_only": deflate(data, strategy=zlib.Z_HUFFMAN_ONLY),
        "odd_rle": deflate(data, strategy=zlib.Z_RLE),
        "odd_sync_flushed": flushed(data, 30000, zlib.Z_SYNC_FLUSH),
        "odd_full_flushed": flushed(data, 50000, zlib.Z_FULL_FLUSH),
        "odd_members": b"".join(gzip.compress(data[a:b], 5, mtime=0) for a, b in zip(cuts, cuts[1:])),
        "odd_empty_member_first": gzip.compress(b"", 6, mtime=0) + gzip.compress(data, 6, mtime=0),
        "odd_trailing_garbage": gzip.compress(data, 6, mtime=0) + b"\0" * 100,
        "odd_control_chars": gzip.compress(data.replace(b"@read_7 ", b"@read_7\x01\x02 ", 1), 6, mtime=0),
        "odd_1000_to_1": gzip.compress(b"@r\n" + b"A" * 3000000 + b"\n+\n" + b"I" * 3000000 + b"\n", 6, mtime=0),
    })

    rng = np.random.RandomState(13)
    data = T.read_like_fastq(rng, 200, 4000)
    half = len(data) // 2
    c.update({
        "bgzf": T.bgzf(data),
        "bgzf_small_blocks": T.bgzf(data, 700, 1),
        "bgzf_then_plain": T.bgzf(data[:half]) + gzip.compress(data[half:], 6, mtime=0),
        "plain_then_bgzf": gzip.compress(data[:half], 6, mtime=0) + T.bgzf(data[half:]),
        "bgzf_garbage_behind": T.bgzf(data) + b"\0\0\0",
    })
    blob = T.bgzf(data)
    for k in range(6):
        b = bytearray(blob)
        b[int(rng.randint(30, len(b) - 30))] ^= 1 << int(rng.randint(8))
        c["bgzf_flip%d" % k] = bytes(b)

    rng = np.random.RandomState(5)
    blob = bytearray(gzip.compress(T.read_like_fastq(rng, 120, 3000), 6, mtime=0))
    for k in range(8):
        c["cut%d" % k] = bytes(blob[:int(rng.randint(20, len(blob)))])
    for k in range(12):
        b = bytearray(blob)
        b[int(rng.randint(10, len(b) - 8))] ^= 1 << int(rng.randint(8))
        c["flip%d" % k] = bytes(b)
    b = bytearray(blob); b[-8] ^= 0x55; c["crc"] = bytes(b)
    b = bytearray(blob); b[-1] ^= 0x01; c["isize"] = bytes(b)

    blob = _bgzf.zlib_bgzf(_cases.c1_fastq_bytes(n=400), 6)
    ms = _bgzf.validate(blob)[1]["members"]
    c["dev_good"] = blob
    c["dev_no_eof_block"] = blob[:-28]
    for how in ("bit", "crc", "isize", "cut_in_member", "cut_at_boundary", "bsize", "plain_member_behind", "garbage_behind_eof", "first_member"):
        at, size, _ = ms[0 if how == "first_member" else len(ms) // 2]
        b = bytearray(blob)
        if how in ("bit", "first_member"):
            b[at + 18 + (size - 26) // 2] ^= 0x04
        elif how == "crc":
            b[at + size - 7] ^= 0x40
        elif how == "isize":
            b[at + size - 4:at + size] = struct.pack("<I", struct.unpack_from("<I", b, at + size - 4)[0] - 1)
        elif how == "cut_in_member":
            b = b[:at + size // 2]
        elif how == "cut_at_boundary":
            b = b[:at]
        elif how == "bsize":
            b[at + 16:at + 18] = struct.pack("<H", 0xfff0)
        elif how == "plain_member_behind":
            b = b[:at] + gzip.compress(b"@x\nACGT\n+\n!!!!\n")
        else:
            b = b + b"\x1f\x8bgarbage behind the end-of-file block"
        c["dev_" + how] = bytes(b)
    # A BSIZE too small for the member's own header and trailer: a gzip member like any other, zlib reads it.  The reader before the
    # layers were separated took it for BGZF in one place and not in the other and ended in an error: expected to differ.
    for k in (0, len(ms) // 2):
        b = bytearray(blob)
        b[ms[k][0] + 16:ms[k][0] + 18] = struct.pack("<H", 20)
        c["fixed_bsize_below_header_%d" % k] = bytes(b)
    return c


def build(tree, out):
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-pthread", "-I" + os.path.join(tree, "filtlong_amd", "csrc"),
                           "-I" + os.path.join(tree, "filtlong_amd", "cli"), "-o", out, os.path.join(ROOT, "tests", "pinflate_layers_host.cpp"), "-lz"])
    return out


def trace(exe, path, chunk, threads, device, nozlib):
    env = dict(os.environ, FLX_CLI_PINFLATE_MIN="1", FLX_CLI_PINFLATE_CHUNK=str(chunk), FLX_CLI_PINFLATE_TIMING="1")
    env.pop("FLX_CLI_PINFLATE", None)
    if nozlib:
        env["FLX_CLI_PINFLATE"] = "nozlib"
    r = subprocess.run([exe, path, str(threads), "70000", "50000"] + (["device"] if device else []), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       env=env, timeout=300)
    err = re.sub(r"search .* s, ", "", r.stderr.decode())
    err = re.sub(r", [0-9.]+ ms in flx_bgzf_inflate", "", err)
    return "exit %d\n%s%s" % (r.returncode, r.stdout.decode(), err)


def main():
    other = sys.argv[1]
    work = sys.argv[2] if len(sys.argv) > 2 else tempfile.mkdtemp(prefix="pinflate_trace_")
    os.makedirs(work, exist_ok=True)
    here, there = build(ROOT, os.path.join(work, "trace_this")), build(other, os.path.join(work, "trace_other"))
    cases = []
    for name, blob in sorted(corpus().items()):
        path = os.path.join(work, name + ".gz")
        with open(path, "wb") as f:
            f.write(blob)
        for chunk in (700, 4096, 65536):
            for threads in (2, 5, 16):
                for device in (False, True):
                    cases.append((name, path, chunk, threads, device, False))
                if name.startswith("level"):
                    cases.append((name, path, chunk, threads, False, True))
    with concurrent.futures.ThreadPoolExecutor(8) as pool:
        a = list(pool.map(lambda c: trace(here, *c[1:]), cases))
        b = list(pool.map(lambda c: trace(there, *c[1:]), cases))
        differ, timing = [], []
        expected = [c for c, x, y in zip(cases, a, b) if x != y and c[0].startswith("fixed_")]
        print("%d cases of %d differ as expected (fixed_*)" % (len(expected), sum(c[0].startswith("fixed_") for c in cases)))
        for c in [c for c, x, y in zip(cases, a, b) if x != y and not c[0].startswith("fixed_")]:
            # a trace that depends on timing (an access point at the very end of the stream is kept only if the reader has it before
            # the last bytes are copied): the same few traces must come out of both builds when each runs many times at once
            many = [set(pool.map(lambda _: trace(exe, *c[1:]), range(24))) for exe in (here, there)]
            (timing if many[0] == many[1] and len(many[0]) > 1 else differ).append(c)
    for c in timing:
        print("depends on timing, the same traces from both builds: %s chunk %d threads %d device %d nozlib %d" % (c[0], c[2], c[3], c[4], c[5]))
    lines = sum(x.count("\n") for x in a)
    points = sum(x.count("\npoint ") for x in a)
    print("%d cases over %d files compared (%d lines, %d access points), %d differ" % (len(cases), len(set(c[0] for c in cases)), lines, points, len(differ)))
    for c in differ:
        print("DIFFERS: %s chunk %d threads %d device %d nozlib %d" % (c[0], c[2], c[3], c[4], c[5]))
    if differ:
        c = differ[0]
        x, y = trace(here, *c[1:]).split("\n"), trace(there, *c[1:]).split("\n")
        for l, m in zip(x, y):
            if l != m:
                print(" this : " + l + "\n other: " + m)
                break
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
