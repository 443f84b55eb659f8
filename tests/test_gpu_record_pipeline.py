"""The record-layout pass that flx_bam_to_fastq_dev and flx_bam_from_fastq_dev share (csrc/record_pipeline.h), where tens of records
cannot reach: record counts on both sides of a tile of 256 records, and 65793 records (258 tiles: the scan over the tiles goes
round twice and the last tile holds one record).  Tiny records of 1 to 20 bases, compared byte for byte, offsets included, with
the models of tests/_bam.py and tests/_bam_encode_cases.py.  The larger cases carry skipped records on both sides of a tile border,
one read of 4097 bases (two emit items, so the items behind it are not numbered like their records) and damaged records in the
first and the last tile.  One Bgzf object goes through a sequence of calls that makes every buffer of its slot grow and be reused."""
import gzip
import random

import pytest

import _bam
import _bam_encode_cases as enc
from filtlong_amd import api
from test_gpu_bam import to_fastq_dev
from test_gpu_bam_encode import from_fastq_dev

pytestmark = pytest.mark.gpu

TILE = 256
COUNTS = (255, 256, 257, 65793)
LONG_AT = 100  # the record of 4097 bases


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


def skipped_at(n):
    """records without text on both sides of a tile border: the first one and, where the count reaches it, the one at which the
    scan over the tiles begins its second round"""
    return {k for border in (TILE, TILE * TILE) for k in (border - 1, border) if k < n}


def bam_records(n):
    rng = random.Random(n)
    skip = skipped_at(n) if n > TILE else set()
    out = []
    for k in range(n):
        l = 4097 if (n > TILE and k == LONG_AT) else rng.randrange(1, 21)
        flag = 4 | (0x10 if rng.random() < 0.3 else 0) | (rng.choice((0x100, 0x800)) if k in skip and k % 2 else 0)
        seq = "" if k in skip and not k % 2 else "".join(rng.choice("ACGTN") for _ in range(l))
        qual = None if rng.random() < 0.05 else bytes(rng.randrange(0, 100) for _ in range(len(seq)))
        out.append(_bam.rec(enc.rname(rng, 1 + k % 6), seq, qual, flag))
    return out


def text_entries(n):
    rng = random.Random(-n)
    out = []
    for k in range(n):
        l = 4097 if (n > TILE and k == LONG_AT) else rng.randrange(1, 21)
        header = enc.rname(rng, 1 + k % 6) + (b" c" if k % 5 == 0 else b"")
        fasta = rng.random() < 0.3
        out.append((b">" if fasta else b"@", header, enc.rseq(rng, l, b"ACGTNacgt"), b"" if fasta else enc.rqual(rng, l)))
    return out


@pytest.fixture(scope="module")
def decode_cases():
    """{count: (records, BAM bytes, record offsets, (text, text offsets, skipped))}: computed once, shared, never changed"""
    out = {}
    for n in COUNTS:
        recs = bam_records(n)
        out[n] = (recs, _bam.bam_bytes(recs), _bam.record_offsets(recs), _bam.expected_fastq(recs))
    return out


@pytest.fixture(scope="module")
def encode_cases():
    """{count: (entries, text, record offsets, (BAM bytes, BAM offsets))}: computed once, shared, never changed"""
    out = {}
    for n in COUNTS:
        entries = text_entries(n)
        out[n] = (entries,) + enc.text_of(entries) + (enc.expected_bam(entries),)
    return out


def last_tile(n):
    return (n - 1) // TILE * TILE


@pytest.mark.parametrize("n", COUNTS)
def test_decode_counts(ctx, decode_cases, n):
    recs, blob, rec_off, (want_text, want_off, want_skipped) = decode_cases[n]
    if n > TILE:
        assert want_skipped == len(skipped_at(n)) >= 2 and len(recs[LONG_AT]["seq"]) == 4097
    text, off, skipped, first_bad = to_fastq_dev(ctx, blob, rec_off)
    assert (first_bad, skipped) == (n, want_skipped)
    assert off == want_off
    assert text == want_text
    assert to_fastq_dev(ctx, blob, rec_off, out_cap=len(want_text))[0] == want_text  # exactly enough
    with pytest.raises(api.FlxError) as e:  # (to_fastq_dev checks that nothing at all was written)
        to_fastq_dev(ctx, blob, rec_off, out_cap=len(want_text) - 1)
    assert e.value.code == 5 and e.value.needed == len(want_text)


@pytest.mark.parametrize("n", COUNTS[2:])
def test_decode_bad_records_in_late_tiles(ctx, decode_cases, n):
    """a damaged record gives no text and is no skipped record; the lowest one is first_bad, whichever tile it is in; the text of
    the records in front of it is theirs, and to_fastq_dev checks that nothing is written outside [0, out_len) of the output"""
    recs, blob, rec_off, (want_text, want_off, want_skipped) = decode_cases[n]
    for bad in ((n - 1,), (7, n - 1), (last_tile(n) - 3, n - 1)):
        damaged = bytearray(blob)
        for k in bad:
            damaged[rec_off[k]:rec_off[k] + 36] = _bam.record_bytes(recs[k], l_seq=-1)[:36]
        text, off, skipped, first_bad = to_fastq_dev(ctx, bytes(damaged), rec_off)
        lost = sum(want_off[k + 1] - want_off[k] for k in bad)
        now_bad = sum(not _bam.has_text(recs[k]) for k in bad)  # (the last of 257 records is one of the skipped ones)
        assert first_bad == bad[0] and skipped == want_skipped - now_bad and len(text) == len(want_text) - lost == off[-1], bad
        assert off[:bad[0] + 1] == want_off[:bad[0] + 1] and text[:off[bad[0]]] == want_text[:want_off[bad[0]]], bad


@pytest.mark.parametrize("n", COUNTS)
def test_encode_counts(ctx, encode_cases, n):
    entries, text, rec_off, (want, want_off) = encode_cases[n]
    if n > TILE:
        assert len(entries[LONG_AT][2]) == 4097
    got, off, first_bad = from_fastq_dev(ctx, text, rec_off)
    assert first_bad == n
    assert off == want_off
    assert got == want
    assert from_fastq_dev(ctx, text, rec_off, out_cap=len(want))[0] == want  # exactly enough
    with pytest.raises(api.FlxError) as e:  # (from_fastq_dev checks that nothing at all was written)
        from_fastq_dev(ctx, text, rec_off, out_cap=len(want) - 1)
    assert e.value.code == 5 and e.value.needed == len(want)


@pytest.mark.parametrize("n", COUNTS[2:])
def test_encode_bad_records_in_late_tiles(ctx, encode_cases, n):
    """a record whose shape is not valid (found by the sizes pass: its header line loses its mark) and a QUAL byte out of range
    (found by the emit pass): the lowest one is first_bad, whichever tile it is in and whichever pass finds it; from_fastq_dev
    checks that nothing is written outside the output"""
    entries, text, rec_off, (want, want_off) = encode_cases[n]
    fastq = next(k for k in range(3, TILE) if entries[k][0] == b"@")
    for bad in ((n - 1,), (fastq, n - 1), (last_tile(n) - 3, n - 1)):
        damaged = bytearray(text)
        for k in bad:
            if k == fastq:
                damaged[rec_off[k + 1] - 2] = 127  # the last QUAL byte
            else:
                damaged[rec_off[k]] = ord("#")
        got, off, first_bad = from_fastq_dev(ctx, bytes(damaged), rec_off)
        assert first_bad == bad[0], bad
        assert off[:bad[0] + 1] == want_off[:bad[0] + 1] and got[:off[bad[0]]] == want[:want_off[bad[0]]], bad


def test_slot_buffers_grow_and_are_reused(ctx, encode_cases):
    """one slot (the calls come one after the other, so each takes the first of the two) through calls that ask more of its buffers
    each time, and then less: the compressor's buffers, the encoder's at their first size, its text buffers behind a record larger
    than the slot, its record tables behind pieces of more than 4096 records; every output against zlib and the models"""
    slot = 65280
    rng = random.Random(5)
    plain = bytes(rng.randrange(64) for _ in range(3 * slot + 17))
    entries, text, rec_off, (want, want_off) = encode_cases[65793]
    small = entries[:3000]  # about two pieces of whole records
    big = [small[0], (b"@", b"big", enc.rseq(rng, 2 * slot), enc.rqual(rng, 2 * slot)), small[1]]
    many = [(b">", b"a", b"A", b"")] * 30000  # 5 bytes each: 13056 records to a piece
    z = api.Bgzf(ctx, slot_bytes=slot, slots=2)
    try:
        assert gzip.decompress(z.compress(plain)) == plain
        for case in (small, big, many, small):
            t, off = enc.text_of(case)
            out = api.bgzf_bam_from_fastq(z, t, off)
            model = enc.expected_bam(case)[0]
            assert out.endswith(_bam.EOF_BLOCK) and gzip.decompress(out) == model
            data, first_bad = z.inflate(out)
            assert data == model and first_bad == len(api.bgzf_index(out)[0]) - 1
        assert gzip.decompress(z.compress(plain[:slot + 1], eof=False)) == plain[:slot + 1]
    finally:
        z.close()
