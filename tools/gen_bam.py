#!/usr/bin/env python3
"""FASTQ to unaligned BAM with Python's zlib, so that a BAM input exists where samtools does not: four-line FASTQ records become
records with flag 4 (unmapped), no CIGAR and no tags, in BGZF members of at most 65280 bytes with the `BC` field, and the
end-of-file block.  The whole header line behind the '@' is the read name when it fits BAM's 254 bytes (so the text comes back byte
for byte), else its first word.

    python3 tools/gen_bam.py IN.fastq OUT.bam [--level 1] [--procs 16]
"""
import argparse
import multiprocessing
import struct
import sys
import zlib

import numpy as np

MEMBER = 65280
CODE = np.full(256, 15, dtype=np.uint8)  # anything that is no IUPAC letter: N
for _i, _c in enumerate("=ACMGRSVTWYHKDBN"):
    CODE[ord(_c)] = _i
    CODE[ord(_c.lower())] = _i
HEADER_TEXT = b"@HD\tVN:1.6\tSO:unknown\n"


def header():
    return b"BAM\1" + struct.pack("<i", len(HEADER_TEXT)) + HEADER_TEXT + struct.pack("<i", 0)


def record(name, seq, qual):
    """name: bytes; seq, qual: uint8 arrays of the FASTQ lines' characters"""
    l = len(seq)
    codes = CODE[seq]
    if l & 1:
        codes = np.append(codes, np.uint8(0))
    packed = (codes[0::2] << 4 | codes[1::2]).astype(np.uint8)
    body = (struct.pack("<iiBBHHHiiii", -1, -1, len(name) + 1, 0, 4680, 0, 4, l, -1, -1, 0) + name + b"\0" + packed.tobytes() +
            (qual - 33).astype(np.uint8).tobytes())
    return struct.pack("<I", len(body)) + body


def fastq_records(fq):
    """(name, seq, qual) of a four-line FASTQ held in memory"""
    buf = np.frombuffer(fq, dtype=np.uint8)
    at, n = 0, len(fq)
    while at < n:
        e0 = fq.index(b"\n", at)
        e1 = fq.index(b"\n", e0 + 1)
        e2 = fq.index(b"\n", e1 + 1)
        e3 = fq.find(b"\n", e2 + 1)
        if e3 < 0:
            e3 = n
        if fq[at:at + 1] != b"@" or fq[e1 + 1:e1 + 2] != b"+" or e3 - e2 != e1 - e0:
            raise ValueError("not a four-line FASTQ record at byte %d" % at)
        name = fq[at + 1:e0]
        if len(name) > 254:
            name = name.split()[0][:254]
        yield name, buf[e0 + 1:e1], buf[e2 + 1:e3]
        at = e3 + 1


def fastq_to_bam(fq):
    """the inflated BAM file of a FASTQ text"""
    return header() + b"".join(record(*r) for r in fastq_records(fq))


def member(data, level=1):
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    body = c.compress(data) + c.flush()
    return (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", 18 + len(body) + 8 - 1) + body +
            struct.pack("<II", zlib.crc32(data) & 0xffffffff, len(data)))


def _members(args):
    data, level = args
    return b"".join(member(data[at:at + MEMBER], level) for at in range(0, len(data), MEMBER))


def bgzf(data, level=1, procs=1):
    step = MEMBER * 256
    parts = [(data[at:at + step], level) for at in range(0, len(data), step)]
    if procs > 1 and len(parts) > 1:
        with multiprocessing.Pool(procs) as pool:
            out = pool.map(_members, parts)
    else:
        out = [_members(p) for p in parts]
    return b"".join(out) + member(b"", level)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("fastq")
    ap.add_argument("out")
    ap.add_argument("--level", type=int, default=1)
    ap.add_argument("--procs", type=int, default=min(16, multiprocessing.cpu_count()))
    a = ap.parse_args(argv)
    bam = fastq_to_bam(open(a.fastq, "rb").read())
    blob = bgzf(bam, a.level, a.procs)
    with open(a.out, "wb") as f:
        f.write(blob)
    print("%s: %d bytes of BAM in %d bytes of BGZF" % (a.out, len(bam), len(blob)), file=sys.stderr)


if __name__ == "__main__":
    main()
