"""Unaligned BAM records turned into FASTQ text on the GPU (flx_bam_to_fastq_dev, flx_bam_to_fastq): the whole corpus of
tests/_bam_cases.py gives the text, the text offsets and the skip count tests/_bam.py expects, and the bytes of the host program
(tests/bam_host.cpp) — at every alignment of the input and the output buffer; FLX_ERR_CAPACITY names the length needed; no records
is a no-op; a record the device finds invalid is first_bad; the host-to-host call in several pieces and with a record larger than
its staging."""
import os
import re

import numpy as np
import pytest

import _bam
import _bam_cases as cases
from filtlong_amd import api
from test_bam_host import BUILDS, build_host_program, run_host_program

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def corpus():
    return cases.corpus()


@pytest.fixture(scope="module")
def host_results(corpus, tmp_path_factory):
    d = tmp_path_factory.mktemp("bam_host")
    return run_host_program(build_host_program(BUILDS["O2"], str(d / "bam_host")), d, [cases.case_bam(c) for c in corpus])


def to_fastq_dev(ctx, blob, rec_off, in_shift=0, out_shift=0, out_cap=None):
    """-> (text, text offsets, skipped, first_bad); the output buffer is 0xAB where the kernel wrote nothing"""
    import torch
    n = len(rec_off) - 1
    d_in = torch.zeros(len(blob) + 64, dtype=torch.uint8, device="cuda")
    d_in[in_shift:in_shift + len(blob)] = torch.from_numpy(np.frombuffer(blob, dtype=np.uint8).copy()).to("cuda")
    d_ro = torch.from_numpy(np.asarray(rec_off, dtype=np.uint64).view(np.int64)).to("cuda")
    cap = 2 * (int(rec_off[-1]) - int(rec_off[0])) if out_cap is None else out_cap
    d_out = torch.full((cap + 64,), 0xAB, dtype=torch.uint8, device="cuda")
    d_oo = torch.full((n + 2,), -7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    try:
        out_len, skipped, first_bad = ctx.bam_to_fastq_dev(d_in.data_ptr() + in_shift, len(blob), d_ro.data_ptr(), n, d_out.data_ptr() + out_shift,
                                                           cap, d_oo.data_ptr())
    except api.FlxError:
        assert (d_out.cpu().numpy() == 0xAB).all()  # an error: nothing was written
        raise
    out = d_out.cpu().numpy()
    oo = d_oo.cpu().numpy()
    assert oo[n + 1] == -7 and (out[:out_shift] == 0xAB).all() and (out[out_shift + out_len:] == 0xAB).all()
    return out[out_shift:out_shift + out_len].tobytes(), [int(x) for x in oo[:n + 1]], skipped, first_bad


def test_chunk_size_is_the_one_the_corpus_is_built_around():
    csrc = os.path.join(ROOT, "filtlong_amd", "csrc")
    shared, src = open(os.path.join(csrc, "record_pipeline.h")).read(), open(os.path.join(csrc, "bam.hip")).read()
    assert re.search(r"\bNT = 256;", shared) and re.search(r"\bCHUNK = 16 \* NT;", shared) and cases.EMIT_CHUNK == 16 * 256
    assert re.search(r"BAM_NT = recpipe::NT;", src) and re.search(r"BAM_CHUNK = recpipe::CHUNK;", src)


def test_corpus_dev(ctx, corpus, host_results):
    for c, h in zip(corpus, host_results):
        blob = cases.case_bam(c)
        rec_off = _bam.record_offsets(c.records, **c.header)
        want_text, want_off, want_skipped = _bam.expected_fastq(c.records)
        text, off, skipped, first_bad = to_fastq_dev(ctx, blob, rec_off)
        assert first_bad == len(c.records) and skipped == want_skipped, c.name
        if c.records:
            assert off == want_off, c.name
        assert text == want_text, c.name
        assert text == h[3] and (not c.records or off == h[4]) and skipped == h[2], c.name


def test_every_alignment_of_the_buffers(ctx, corpus):
    by_name = {c.name: c for c in corpus}
    # input shifts 1..15, each with one output shift (5 * shift mod 16: all of 1..15 occur, not every pair); the two records of
    # 300 000 bases, whose reversed 16-byte groups cross chunk borders, at three shifts each
    for name, shifts in (("lengths", range(1, 16)), ("names", range(1, 16)), ("qualities", range(1, 16)), ("bases", range(1, 16)),
                         ("long", (1, 6, 15)), ("long_reverse", (3, 8, 13))):
        c = by_name[name]
        blob = cases.case_bam(c)
        rec_off = _bam.record_offsets(c.records, **c.header)
        want = _bam.expected_fastq(c.records)[0]
        for shift in shifts:
            assert to_fastq_dev(ctx, blob, rec_off, in_shift=shift, out_shift=(5 * shift) % 16)[0] == want, (name, shift)


def test_capacity_and_no_records(ctx, corpus):
    c = {c.name: c for c in corpus}["names"]
    blob = cases.case_bam(c)
    rec_off = _bam.record_offsets(c.records, **c.header)
    want = _bam.expected_fastq(c.records)[0]
    assert to_fastq_dev(ctx, blob, rec_off, out_cap=len(want))[0] == want  # exactly enough
    with pytest.raises(api.FlxError) as e:
        to_fastq_dev(ctx, blob, rec_off, out_cap=len(want) - 1)
    assert e.value.code == 5 and e.value.needed == len(want)  # FLX_ERR_CAPACITY
    with pytest.raises(api.FlxError) as e:
        to_fastq_dev(ctx, blob, rec_off, out_cap=32)
    assert e.value.code == 5 and e.value.needed == len(want)
    assert ctx.bam_to_fastq_dev(None, 0, None, 0, None, 0, None) == (0, 0, 0)  # n_records == 0: a no-op
    head = _bam.header_bytes()
    assert api.bam_to_fastq(ctx, head, with_offsets=True)[0::2] == (b"", 0)


def test_invalid_records_are_first_bad(ctx):
    """damaged records are data both paths refuse cleanly: with the offsets of the good file, the device names the lowest record
    that does not hold inside its range, and stays inside the buffers"""
    recs = cases.three_records() * 3
    good = _bam.bam_bytes(recs)
    rec_off = _bam.record_offsets(recs)
    for k in (0, 4, 8):
        for field, value in (("block_size", 31), ("l_read_name", 0), ("l_seq", -1), ("l_seq", 2 ** 31 - 1), ("n_cigar_op", 65535)):
            bad = bytearray(good)
            raw = _bam.record_bytes(recs[k], **{field: value})
            bad[rec_off[k]:rec_off[k] + 36] = raw[:36]
            text, off, skipped, first_bad = to_fastq_dev(ctx, bytes(bad), rec_off)
            assert first_bad == k, (k, field)
    # offsets that do not follow the records: a record longer or shorter than its range is bad, the others are not touched
    shifted = list(rec_off)
    shifted[5] += 1
    assert to_fastq_dev(ctx, good, shifted)[3] == 4
    past = list(rec_off)
    past[-1] += 40
    assert to_fastq_dev(ctx, good, past)[3] == len(recs) - 1


def test_host_to_host(ctx, corpus):
    for c in corpus:
        want_text, want_off, want_skipped = _bam.expected_fastq(c.records)
        text, off, skipped = api.bam_to_fastq(ctx, cases.case_bam(c), with_offsets=True)
        assert (text, [int(x) for x in off], skipped) == (want_text, want_off, want_skipped), c.name


def test_host_to_host_in_pieces(ctx, corpus):
    by_name = {c.name: c for c in corpus}
    # several pieces of whole records: a staging of 300 bytes takes a few records of "names" at a time, and the records of
    # "lengths" beyond it (and the 300 000-base record of "long", behind a small one) make it grow
    for name, piece in (("names", 300), ("lengths", 300), ("lengths", 5000), ("long", 1000), ("skip_middle_empty", 64)):
        c = by_name[name]
        want_text, want_off, want_skipped = _bam.expected_fastq(c.records)
        text, off, skipped = api.bam_to_fastq(ctx, cases.case_bam(c), piece_bytes=piece, with_offsets=True)
        assert (text, [int(x) for x in off], skipped) == (want_text, want_off, want_skipped), (name, piece)
    c = by_name["names"]
    want = _bam.expected_fastq(c.records)[0]
    with pytest.raises(api.FlxError) as e:
        api.bam_to_fastq(ctx, cases.case_bam(c), piece_bytes=300, out_cap=len(want) - 1)
    assert e.value.code == 5 and e.value.needed == len(want)
    with pytest.raises(ValueError):
        api.bam_to_fastq(ctx, cases.case_bam(c)[:-3])
