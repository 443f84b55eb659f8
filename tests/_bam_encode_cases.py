"""The text corpus of the BAM writer's tests: the smallest shapes at which an encoder can go wrong.  A case is a list of entries
(kind, header, seq, qual): kind b"@" (FASTQ) or b">" (FASTA), the header line, SEQ and QUAL as bytes.  text_of() writes the strict
record text and its offsets; expected_records() gives the record dicts of tests/_bam.py, whose independent writer (record_bytes)
says what the bytes must be.  damaged() -> record texts that break one rule each."""
import functools
import random
from collections import namedtuple

import _bam

ENC_CHUNK = 4096  # bases per emit item of csrc/bam_encode.hip (test_gpu_bam_encode.py checks the source says so)
LENGTHS = [0, 1, 2, 15, 16, 17, 31, 32, 33, ENC_CHUNK - 1, ENC_CHUNK, ENC_CHUNK + 1, 2 * ENC_CHUNK + 1]
LONG = 300_000

Case = namedtuple("Case", "name entries")


def text_of(entries):
    """(text, rec_off)"""
    text, off = bytearray(), [0]
    for kind, header, seq, qual in entries:
        text += kind + header + b"\n" + seq + b"\n"
        if kind == b"@":
            assert len(qual) == len(seq)
            text += b"+\n" + qual + b"\n"
        off.append(len(text))
    return bytes(text), off


def name_of_header(header):
    cut = [i for i, c in enumerate(header) if c in b" \t"]
    return header[:cut[0]] if cut else header


def base_of(c):
    ch = chr(c).upper() if 97 <= c <= 122 else chr(c)
    return ch if ch in _bam.BASES else "N"


def expected_records(entries):
    return [_bam.rec(name_of_header(h), "".join(base_of(c) for c in s), None if kind == b">" else bytes(c - 33 for c in q))
            for kind, h, s, q in entries]


def expected_bam(entries):
    """(the BAM records, their offsets)"""
    out, off = bytearray(), [0]
    for r in expected_records(entries):
        out += _bam.record_bytes(r)
        off.append(len(out))
    return bytes(out), off


def rname(rng, n):
    return bytes(rng.choice(b"abcdefghijklmnopqrstuvwxyz0123456789_-/:") for _ in range(n))


def rseq(rng, n, alphabet=b"ACGT"):
    return bytes(rng.choice(alphabet) for _ in range(n))


def rqual(rng, n):
    return bytes(rng.choice((33, 126)) if rng.random() < 0.1 else rng.randrange(35, 90) for _ in range(n))


@functools.lru_cache(maxsize=None)
def corpus():
    rng = random.Random(20250319)
    cases = []

    def fq(header, l, alphabet=b"ACGT"):
        return (b"@", header, rseq(rng, l, alphabet), rqual(rng, l))

    def fa(header, l, alphabet=b"ACGT"):
        return (b">", header, rseq(rng, l, alphabet), b"")

    # every length, names of 1..16 bytes in turn so that record, sequence and output starts fall on every alignment
    cases.append(Case("lengths", [fq(rname(rng, 1 + i % 16), l) for i, l in enumerate(LENGTHS + LENGTHS[::-1])]))
    cases.append(Case("lengths_fasta", [fa(rname(rng, 1 + (3 * i) % 16), l) for i, l in enumerate(LENGTHS)]))
    cases.append(Case("long", [fq(b"short_before", 4), fq(b"long_read", LONG), fq(b"odd_behind", 33)]))
    # names of 1 and 254 bytes; headers with blank and tab comments (the comment is not stored)
    cases.append(Case("names", [fq(b"x", 4), fq(rname(rng, 254), 100), fq(rname(rng, 254) + b" a comment", 7),
                                fq(b"n1 comment with blanks", 20), fq(b"n2\ttab comment", 21), fq(b"n3 \t both", 22), fa(b"y", 0),
                                fa(b"f1 comment", 19), fa(b"f2\tcomment ", 18)] +
                      [fq(rname(rng, k) + (b" c" if k % 2 else b""), 17 + 3 * k) for k in range(1, 17)]))
    # all 256 byte values in SEQ except '\n', at even and odd positions
    every = bytes(c for c in range(256) if c != 10)
    cases.append(Case("bases", [(b"@", b"all", every, rqual(rng, len(every))), (b"@", b"all_odd", b"A" + every, rqual(rng, len(every) + 1)),
                                (b">", b"all_fasta", every[::-1], b""), (b"@", b"iupac", b"=ACMGRSVTWYHKDBNacmgrsvtwyhkdbn", rqual(rng, 31))]))
    # qualities: 33 and 126 at every position of a 16-byte group and of the head and tail bytes
    edge = bytes([33, 126] * 40)
    cases.append(Case("qualities", [(b"@", b"edges", rseq(rng, 80), edge), (b"@", b"edges_odd", rseq(rng, 79), edge[1:]),
                                    (b"@", b"all33", rseq(rng, 50), b"!" * 50), (b"@", b"all126", rseq(rng, 51), b"~" * 51)]))
    # a mix of both kinds; an odd L as the last record (its low pad nibble must be zero)
    cases.append(Case("mixed", [fq(b"q1 c", 40), fa(b"a1", 41), fq(b"q2", 0), fa(b"a2 c", 1), fa(b"a3", ENC_CHUNK + 1), fq(b"q3", 2 * ENC_CHUNK + 1),
                                fa(b"last_odd", 77, b"ACGTN")]))
    cases.append(Case("last_odd_fastq", [fq(b"only", 16 * 5 + 33, b"T")]))
    cases.append(Case("no_records", []))
    return tuple(cases)


def damaged():
    """[(name, text, rec_off, first_bad)]: three good records with the middle one (record 1) broken"""
    rng = random.Random(7)
    good = [(b"@", b"r0 c", rseq(rng, 40), rqual(rng, 40)), (b"@", b"r1", rseq(rng, 37), rqual(rng, 37)), (b">", b"r2", rseq(rng, 30), b"")]
    text, off = text_of(good)
    out = []

    def broken(name, middle):
        t = text[:off[1]] + middle + text[off[2]:]
        out.append((name, t, [0, off[1], off[1] + len(middle), off[1] + len(middle) + off[3] - off[2]], 1))

    kind, h, s, q = good[1]
    broken("missing_plus", b"@" + h + b"\n" + s + b"\n-\n" + q + b"\n")
    broken("odd_remainder", b"@" + h + b"\n" + s + b"\n+\n" + q[:-1] + b"\n")
    broken("newline_not_where_L_puts_it", b"@" + h + b"\n" + s + b"A\n+\n" + q[:-2] + b"\n\n")
    broken("newline_missing_at_end", b"@" + h + b"\n" + s + b"\n+\n" + q + b"!")
    broken("empty_name", b"@\n" + s + b"\n+\n" + q + b"\n")
    broken("empty_name_with_comment", b"@ comment\n" + s + b"\n+\n" + q + b"\n")
    broken("name_255", b"@" + b"n" * 255 + b"\n" + s + b"\n+\n" + q + b"\n")
    broken("no_mark", b"r1\n" + s + b"\n+\n" + q + b"\n\n")
    broken("header_without_end", b"@" + h + s)
    for pos in (0, 1, 15, 16, 17, 36):  # head bytes, whole stores and tail bytes of the quality part
        for v in (32, 127, 10, 200):
            broken("qual_%d_at_%d" % (v, pos), b"@" + h + b"\n" + s + b"\n+\n" + q[:pos] + bytes([v]) + q[pos + 1:] + b"\n")
    broken("fasta_newline_missing", b">" + h + b"\n" + s + b"A")
    out.append(("all_good", text, list(off), 3))
    return out
