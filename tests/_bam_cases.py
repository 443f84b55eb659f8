"""The BAM corpus of the tests: the smallest shapes at which a decoder can go wrong.  corpus() -> [Case]; every case is a few
kilobytes except the one 300 000-base record.  damaged() -> inflated files that are truncated or malformed."""
import functools
import random
import struct
from collections import namedtuple

import _bam

EMIT_CHUNK = 4096  # bases per emit item of csrc/bam.hip (BAM_CHUNK; test_gpu_bam.py checks the source says so)
LENGTHS = [1, 2, 7, 8, 9, 63, 64, 65, EMIT_CHUNK - 1, EMIT_CHUNK, EMIT_CHUNK + 1, 2 * EMIT_CHUNK + 1]
LONG = 300_000
CIGAR3 = (10 << 4 | 4, 5 << 4 | 0, 3 << 4 | 4)  # 10S5M3S
TAGS = b"RGZgroup1\0qsi\x0c\0\0\0mvBc" + struct.pack("<I", 3) + b"\x01\x00\x01"

Case = namedtuple("Case", "name records header")


def random_seq(rng, n, alphabet=_bam.BASES):
    return "".join(rng.choice(alphabet) for _ in range(n))


def random_qual(rng, n):
    return bytes(rng.choice((0, 1, 20, 40, 93)) if rng.random() < 0.1 else rng.randrange(2, 60) for _ in range(n))


def name_of(rng, n):
    return bytes(rng.choice(b"abcdefghijklmnopqrstuvwxyz0123456789_-/:") for _ in range(n))


@functools.lru_cache(maxsize=None)
def corpus():
    rng = random.Random(20240611)
    cases = []

    def add(name, records, **header):
        cases.append(Case(name, records, header))

    # every length, forward and reverse-complemented; names of 1..16 bytes in turn, so that record, sequence and text starts fall
    # on every alignment; CIGAR of 0 and 3 operations and records with and without tags in turn
    recs = []
    for i, l in enumerate(LENGTHS + LENGTHS):
        recs.append(_bam.rec(name_of(rng, 1 + i % 16), random_seq(rng, l), random_qual(rng, l), flag=0x10 if i >= len(LENGTHS) else 4,
                             cigar=CIGAR3 if i % 3 == 1 else (), tags=TAGS if i % 2 else b""))
    add("lengths", recs)
    add("long", [_bam.rec(b"short_before", "ACGT", bytes([30] * 4)),
                 _bam.rec(b"long_forward", random_seq(rng, LONG, "ACGT"), random_qual(rng, LONG)),
                 _bam.rec(b"odd_name_", random_seq(rng, 33), random_qual(rng, 33), flag=0x10)])
    add("long_reverse", [_bam.rec(b"r", random_seq(rng, LONG + 1, "ACGTN"), random_qual(rng, LONG + 1), flag=0x10)])
    # names: 1 and 254 bytes, and a run of 1..16 with sequences of 1..40 so that every start alignment mod 16 occurs
    add("names", [_bam.rec(b"x", "ACGT", bytes(4)), _bam.rec(name_of(rng, 254), random_seq(rng, 100), random_qual(rng, 100))] +
        [_bam.rec(name_of(rng, k), random_seq(rng, 17 + 3 * k), random_qual(rng, 17 + 3 * k), flag=(0x10 if k % 2 else 0)) for k in range(1, 17)] +
        [_bam.rec(name_of(rng, 16 - k), random_seq(rng, 40 + k), random_qual(rng, 40 + k), tags=TAGS[:k]) for k in range(0, 16)])
    # all 16 base codes at even and odd positions, both directions
    every = _bam.BASES + _bam.BASES[::-1] + "A" + _bam.BASES
    add("bases", [_bam.rec(b"all16", every, random_qual(rng, len(every))), _bam.rec(b"all16_rc", every, random_qual(rng, len(every)), flag=0x10),
                  _bam.rec(b"all16_odd", every[:-1], random_qual(rng, len(every) - 1), flag=0x10)])
    # qualities: 0, 93, 94, 254, 0xFF in the middle, 0xFF first (missing)
    edge = bytes([0, 93, 94, 254, 1, 0xff, 2, 92] * 9)
    add("qualities", [_bam.rec(b"edges", random_seq(rng, len(edge)), edge), _bam.rec(b"edges_rc", random_seq(rng, len(edge)), edge, flag=0x10),
                      _bam.rec(b"missing", random_seq(rng, 70), None), _bam.rec(b"missing_rc", random_seq(rng, 71), None, flag=0x10),
                      _bam.rec(b"ff_first_only", random_seq(rng, 40), b"\xff" + bytes([30] * 39)),
                      _bam.rec(b"ff_last", random_seq(rng, 40), bytes([30] * 39) + b"\xff")])
    # flags: 0x10 on odd and even lengths (above); 0x100, 0x800 and l_seq == 0 skipped, at the first, a middle and the last place;
    # 0x40 / 0x80 leave the name alone
    keep = lambda k: _bam.rec(b"keep%d" % k, random_seq(rng, 30 + k), random_qual(rng, 30 + k), flag=(0x40 | 0x1 if k % 2 else 0x80 | 0x1))
    for kind, skip in (("secondary", lambda: _bam.rec(b"sec", random_seq(rng, 50), random_qual(rng, 50), flag=0x100)),
                       ("supplementary", lambda: _bam.rec(b"sup", random_seq(rng, 51), random_qual(rng, 51), flag=0x800 | 0x10)),
                       ("empty", lambda: _bam.rec(b"empty", "", b"", tags=TAGS))):
        add("skip_first_" + kind, [skip(), keep(1), keep(2)])
        add("skip_middle_" + kind, [keep(1), skip(), keep(2), keep(3)])
        add("skip_last_" + kind, [keep(1), keep(2), skip()])
    add("skip_all", [_bam.rec(b"a", "", b""), _bam.rec(b"b", "ACGT", bytes(4), flag=0x900)])
    # small files
    add("header_only", [])
    add("header_with_references", [_bam.rec(b"r1", random_seq(rng, 20), random_qual(rng, 20))], refs=((b"chr1", 1000), (b"contig_2", 5)))
    add("header_text_empty", [_bam.rec(b"r1", random_seq(rng, 21), random_qual(rng, 21))], text=b"")
    add("header_only_text_empty", [], text=b"")
    return tuple(cases)


_BLOBS = {}


def case_bam(c):
    """the inflated file of a case"""
    if c.name not in _BLOBS:
        _BLOBS[c.name] = _bam.bam_bytes(c.records, **c.header)
    return _BLOBS[c.name]


def bgzf_layouts(c):
    """{layout: BGZF file} of a case: members of 65280 bytes, small members that records straddle, one member per record (records
    that fit a member), and no end-of-file block"""
    data = case_bam(c)
    out = {"default": _bam.bgzf(data), "no_eof": _bam.bgzf(data, eof=False)}
    if len(data) < 1 << 16:
        out["straddle"] = _bam.bgzf(data, member=61)
        off = _bam.record_offsets(c.records, **c.header)
        if all(b - a <= 65536 for a, b in zip(off, off[1:])):
            out["member_per_record"] = _bam.bgzf(data, cuts=off)
    return out


def three_records():
    rng = random.Random(5)
    return [_bam.rec(b"one", random_seq(rng, 9), random_qual(rng, 9), tags=b"XYZab\0"), _bam.rec(b"two_", random_seq(rng, 16), random_qual(rng, 16), flag=0x10, cigar=CIGAR3),
            _bam.rec(b"three", random_seq(rng, 5), None)]


def damaged():
    """[(name, inflated bytes)]: every truncation point of a three-record file, records that break one rule each, and 200
    single-byte corruptions of the fixed fields.  What each must give is _bam.walk_model's word."""
    recs = three_records()
    good = _bam.bam_bytes(recs, refs=((b"ref", 10),))
    out = [("cut_%d" % n, good[:n]) for n in range(len(good))]
    head = _bam.header_bytes()
    first, last = _bam.record_bytes(recs[0]), _bam.record_bytes(recs[2])

    def with_middle(name, middle):
        out.append((name, head + first + middle + last))
        out.append((name + "_at_end", head + first + middle))

    r = recs[1]
    with_middle("block_size_31", _bam.record_bytes(r, block_size=31))
    with_middle("block_size_short_by_1", _bam.record_bytes(r, block_size=len(_bam.record_bytes(r)) - 4 - 1))
    with_middle("l_read_name_0", _bam.record_bytes(r, l_read_name=0))
    raw = bytearray(_bam.record_bytes(r))
    raw[36 + len(r["name"])] = ord("!")
    with_middle("name_without_nul", bytes(raw))
    for v in (-1, -2 ** 31, 2 ** 31 - 1, 2 ** 31 - 2, 2 ** 30, 65536, 17):
        with_middle("l_seq_%d" % v, _bam.record_bytes(r, l_seq=v))
    for v in (65535, 65534, 32768, 4):
        with_middle("n_cigar_op_%d" % v, _bam.record_bytes(r, n_cigar_op=v))
    with_middle("l_seq_and_n_cigar_large", _bam.record_bytes(r, l_seq=2 ** 31 - 1, n_cigar_op=65535))
    with_middle("block_size_huge", _bam.record_bytes(r, block_size=2 ** 32 - 1))
    out.append(("no_magic", b"BAM\2" + good[4:]))
    out.append(("l_text_negative", b"BAM\1" + struct.pack("<i", -1) + good[8:]))
    out.append(("n_ref_negative", b"BAM\1" + struct.pack("<ii", 0, -5) + good[8:]))
    out.append(("ref_name_negative", b"BAM\1" + struct.pack("<iii", 0, 1, -1) + good[8:]))
    out.append(("n_ref_huge", b"BAM\1" + struct.pack("<ii", 0, 2 ** 31 - 1) + good[8:]))
    rng = random.Random(99)
    off = _bam.record_offsets(recs, refs=((b"ref", 10),))
    fixed = [o + k for o in off[:-1] for k in (0, 1, 2, 3, 12, 16, 17, 18, 19, 20, 21, 22, 23)]  # block_size, l_read_name, n_cigar_op, flag, l_seq
    for i in range(200):
        b = bytearray(good)
        at = rng.choice(fixed + list(range(4, off[0])))
        b[at] ^= 1 << rng.randrange(8)
        out.append(("fuzz_%d" % i, bytes(b)))
    return out
