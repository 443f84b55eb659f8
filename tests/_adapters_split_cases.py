"""Reads and batches for the --split_adapters tests: every placement the definition and the kernels' cutting have.

The constants below mirror csrc/adapters_split.hip and csrc/adapters.h; tests/test_adapters_split_cases.py reads them out of the
sources and compares, so a retuned kernel fails there instead of quietly losing the coverage of its edges."""
import numpy as np

import _adapters_model as model
from _adapters_cases import LIGATION, indel, pack, random_adapter, random_seq, substitute  # noqa: F401

PIECE_BASES = 1024      # S: kPieceBases
WARMUP = 96             # adapters::kWarmup
MAX_PIECES = 28         # kMaxPieces: pieces per workgroup at most
ITEMS_PER_GROUP = 1024  # kItemsPerGroup
MAX_GROUPS = 8192       # kMaxGroups
SPLIT_WAVES = 4         # kSplitWaves: reads per workgroup of the child walk
STEP_BASES = 64 * 32    # bases per wave and step of the child walk


def pieces_per_group(n_patterns):
    return max(1, min(ITEMS_PER_GROUP // n_patterns, MAX_PIECES))


def placements(rng, seqs, split_errors, S=PIECE_BASES):
    """reads whose adapters sit on every edge of a piece of S bases and of its warm-up, for the adapters `seqs`"""
    a = bytes(seqs[0]).upper()
    m = len(a)
    k2 = m * split_errors // 100
    body = lambda n: random_seq(rng, max(n, 0))
    total = 2 * S + 57
    reads = []
    for j in (S - 1, S, S + 1, S + m - 1, S + m, S + m + k2, S + m + k2 + 1, 2 * S, 2 * S + 1, total):  # the adapter ends at j
        reads.append(body(j - m) + a + body(total - j))
    for off in (1, m // 2, m - 1):                          # an occurrence that straddles a piece boundary
        reads.append(body(S - off) + a + body(S))
        reads.append(body(2 * S - off) + model.revcomp(a) + body(40))
    reads.append(body(300) + a + a + body(300))             # back to back
    reads.append(body(300) + a + b"G" + a + body(300))      # one base apart
    reads.append(body(S - m - 1) + a + b"T" + a + body(9))  # ... across a piece boundary
    if len(seqs) > 1:
        b = bytes(seqs[1]).upper()
        reads.append(body(200) + a + b + body(200))         # the marks of two patterns meet and merge
        reads.append(body(200) + a[:m - 3] + b + body(200))
        reads.append(body(S - 5) + b + body(3) + model.revcomp(a) + body(S))
    for s in seqs[:3]:
        s = bytes(s).upper()
        reads.append(body(500) + model.revcomp(s) + body(700))
        reads.append(body(S - 9) + substitute(rng, s, max(1, len(s) // 10)) + body(400))  # 10 % substitutions
        for k in (1, 2, 3):
            reads.append(body(S + 3) + indel(rng, s, k) + body(300))                        # 1-3-base indels
    return reads


def end_rule_reads(rng, seqs):
    """the middle marks against the cuts of the ends rule (W of about 2 m)"""
    a = bytes(seqs[0]).upper()
    m = len(a)
    body = lambda n: random_seq(rng, max(n, 0))
    return [
        a + a + body(500),                      # a mark partly (or wholly) inside the head cut
        body(m // 2) + a + a + body(500),
        body(500) + a + model.revcomp(a),       # a mark reaching past e
        body(500) + a + a[:m // 2],
        a + body(600),                          # an end hit without a middle hit ... (the occurrence itself is a middle hit too)
        body(600) + model.revcomp(a),
        body(400) + a + body(400),              # a middle hit without an end hit
        a * 3,                                  # all adapter
        a,
        a + body(300) + a + body(300) + a,      # everything at once
        body(3) + a + body(2),
    ]


def byte_reads(rng, seqs, S=PIECE_BASES):
    a = bytes(seqs[0]).upper()
    m = len(a)
    body = lambda n: random_seq(rng, max(n, 0))
    every = bytes(range(256))
    mixed = bytearray(body(S - 3) + a + body(300) + a + body(3))
    for i in range(0, len(mixed), 2):
        mixed[i] |= 0x20
    return [
        b"", b"A", b"N", body(m - 1), body(m), body(S - 1), body(S), body(S + 1), body(2 * S), body(2 * S + 1), body(3 * S + 5),
        b"A" * (2 * S + 100),                                   # a homopolymer: long runs of hit ends for a homopolymer-rich pattern
        b"A" * 700 + b"C" + b"A" * 900,
        b"N" * (S + 40), b"N" * 50 + a + b"N" * S,
        (body(S - 10) + a + body(200)).lower(), bytes(mixed),
        every * 5, a[:m // 2] + every + a[m // 2:] + every[::-1] + a,
        bytes(rng.integers(0, 256, size=S + 200, dtype=np.uint8)),
    ]


def chimera(rng, seqs, left, right, which=0):
    return random_seq(rng, left) + bytes(seqs[which]).upper() + random_seq(rng, right)


# ---- how the kernels cut the work ----------------------------------------------------------------------------------------------------
MIRRORED = {"kPieceBases": PIECE_BASES, "kMaxPieces": MAX_PIECES, "kItemsPerGroup": ITEMS_PER_GROUP, "kMaxGroups": MAX_GROUPS,
            "kSplitWaves": SPLIT_WAVES, "kWarmup": WARMUP}


def source_constants():
    """the mirrored constants as csrc/adapters_split.hip and csrc/adapters.h state them"""
    import os
    import re
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "filtlong_amd", "csrc")
    text = open(os.path.join(csrc, "adapters_split.hip")).read() + open(os.path.join(csrc, "adapters.h")).read()
    found = {}
    for name in MIRRORED:
        m = re.search(r"constexpr int %s = (\d+);" % name, text)
        found[name] = int(m.group(1)) if m else None
    return found


GEOMETRY_ADAPTER = b"GATTACAGGCTA"  # 12 bases; with E2 = 0 and N between the occurrences nothing else can hit
PIECE_SETS = (1, 32, 128)          # sequences: 2, 64 and 256 patterns, 28, 16 and 4 pieces a workgroup
PIECE_KINDS = ("below", "exact", "above", "partial")


def piece_total(ppb, kind):
    return {"below": ppb - 1, "exact": ppb, "above": ppb + 1, "partial": 2 * ppb + ppb // 2 + 1}[kind]


def piece_batch(n_seqs, kind, seed=0):
    """(seqs, reads in processing order, pieces per read, pieces per workgroup): a batch of exactly piece_total pieces.  Most pieces
    are short (a piece is work for one lane whatever its length); reads of two and three pieces lie across the workgroup boundaries,
    and an adapter ends inside the last piece in front of every boundary and another inside the first piece behind it."""
    rng = np.random.default_rng(1000 * n_seqs + seed)
    seqs = [GEOMETRY_ADAPTER] + [random_adapter(rng, 12) for _ in range(n_seqs - 1)]
    ppb = pieces_per_group(2 * n_seqs)
    total = piece_total(ppb, kind)
    counts, left, i = [], total, 0
    while left:
        c = min(left, (1, 1, 3, 1, 2, 3, 2)[i % 7])
        counts.append(c)
        left -= c
        i += 1
    reads = []
    for c in counts:
        tail = int(rng.integers(120, 260))
        reads.append(bytearray(random_seq(rng, (c - 1) * PIECE_BASES + tail)))
    start = np.concatenate(([0], np.cumsum(counts)))
    a, m = seqs[0], len(seqs[0])

    def plant(piece, front):  # an occurrence inside global piece `piece`: at its front or at its back
        r = int(np.searchsorted(start, piece, side="right")) - 1
        lo = (piece - int(start[r])) * PIECE_BASES
        hi = min(lo + PIECE_BASES, len(reads[r]))
        at = lo + 20 if front else hi - m - 20
        reads[r][at:at + m] = a

    for b in range(ppb, total, ppb):
        plant(b - 1, False)
        plant(b, True)
    plant(0, True)
    plant(total - 1, False)
    return seqs, [bytes(r) for r in reads], counts, ppb


CHILD_COUNTS = (1, 1023, 1024, 1025)
READ_COUNTS = (255, 256, 257)


def child_count_batch(nc):
    """reads (W = 1: no end hits) of which one has exactly nc children: N N N, then nc - 1 times the adapter and N N N"""
    a = GEOMETRY_ADAPTER
    one = b"NNN" + (a + b"NNN") * (nc - 1) if nc > 1 else b"NNN" + a
    return [b"ACGTNACGT", one, b"", b"N" * 40]


def read_count_batch(n, seed=3):
    """n short reads, every third one a chimera of two 20-base halves; the last read is one"""
    rng = np.random.default_rng(seed)
    reads = [random_seq(rng, int(rng.integers(0, 60))) for _ in range(n)]
    for i in list(range(0, n, 3)) + [n - 1]:
        reads[i] = random_seq(rng, 20) + GEOMETRY_ADAPTER + random_seq(rng, 20)
    return reads
