"""FASTQ / FASTA record text turned into unaligned BAM records on the GPU (flx_bam_from_fastq_dev, flx_bgzf_bam_from_fastq): the
corpus of tests/_bam_encode_cases.py gives the bytes and the offsets of the independent writer in tests/_bam.py and of the host
program (tests/bam_encode_host.cpp) — at every alignment of the input and the output buffer, with nothing written outside the
result; FLX_ERR_CAPACITY names the length needed; no records is a no-op; an invalid record, or an offset that does not follow the
records, is first_bad; the host-to-host call gives BGZF whose decompressed bytes are the same records whatever the slot size, with
the end-of-file block, and from four threads at once."""
import gzip
import os
import re
import threading

import numpy as np
import pytest

import _bam
import _bam_encode_cases as cases
from filtlong_amd import api
from test_bam_encode_host import BUILDS, build_host_program, run_host_program

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
def expected(corpus):
    """{case name: (text, rec_off, BAM bytes, BAM offsets)}: computed once, shared, never changed"""
    out = {}
    for c in corpus:
        text, off = cases.text_of(c.entries)
        out[c.name] = (text, tuple(off)) + tuple(cases.expected_bam(c.entries))
    return out


@pytest.fixture(scope="module")
def host_results(corpus, tmp_path_factory):
    d = tmp_path_factory.mktemp("bamenc_host")
    return run_host_program(build_host_program(BUILDS["O2"], str(d / "bam_encode_host")), d, [cases.text_of(c.entries) for c in corpus])


def from_fastq_dev(ctx, text, rec_off, in_shift=0, out_shift=0, out_cap=None):
    """-> (BAM bytes, offsets, first_bad); both device buffers are 0xAB where nothing may be written"""
    import torch
    n = len(rec_off) - 1
    d_in = torch.full((len(text) + 64,), 0xAB, dtype=torch.uint8, device="cuda")
    if len(text):
        d_in[in_shift:in_shift + len(text)] = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).to("cuda")
    d_ro = torch.from_numpy(np.asarray(rec_off, dtype=np.uint64).view(np.int64)).to("cuda")
    cap = api.bam_from_fastq_bound(len(text), n) if out_cap is None else out_cap
    d_out = torch.full((cap + 64,), 0xAB, dtype=torch.uint8, device="cuda")
    d_oo = torch.full((n + 2,), -7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    try:
        out_len, first_bad = ctx.bam_from_fastq_dev(d_in.data_ptr() + in_shift, len(text), d_ro.data_ptr(), n, d_out.data_ptr() + out_shift,
                                                    cap, d_oo.data_ptr())
    except api.FlxError:
        assert (d_out.cpu().numpy() == 0xAB).all()  # an error: nothing was written
        raise
    out = d_out.cpu().numpy()
    oo = d_oo.cpu().numpy()
    src = d_in.cpu().numpy()
    assert (src[:in_shift] == 0xAB).all() and (src[in_shift + len(text):] == 0xAB).all()
    assert oo[n + 1] == -7 and (out[:out_shift] == 0xAB).all() and (out[out_shift + min(out_len, cap):] == 0xAB).all()
    return out[out_shift:out_shift + out_len].tobytes(), [int(x) for x in oo[:n + 1]], first_bad


def test_chunk_size_is_the_one_the_corpus_is_built_around():
    csrc = os.path.join(ROOT, "filtlong_amd", "csrc")
    shared, src = open(os.path.join(csrc, "record_pipeline.h")).read(), open(os.path.join(csrc, "bam_encode.hip")).read()
    assert re.search(r"\bNT = 256;", shared) and re.search(r"\bCHUNK = 16 \* NT;", shared) and cases.ENC_CHUNK == 16 * 256
    assert re.search(r"ENC_NT = recpipe::NT;", src) and re.search(r"ENC_CHUNK = recpipe::CHUNK;", src)


def test_corpus_dev(ctx, corpus, expected, host_results):
    for c, h in zip(corpus, host_results):
        text, rec_off, want, want_off = expected[c.name]
        if not c.entries:
            continue
        got, off, first_bad = from_fastq_dev(ctx, text, rec_off)
        assert first_bad == len(c.entries) == h[0], c.name
        assert off == want_off == h[2], c.name
        assert got == want, c.name
        assert got == h[1], c.name


def test_every_alignment_of_the_buffers(ctx, expected):
    # input shifts 1..15, each with one output shift (5 * shift mod 16: all of 1..15 occur, not every pair); the 300 000-base record,
    # whose 16-byte groups cross chunk borders, at three shifts
    for name, shifts in (("lengths", range(1, 16)), ("lengths_fasta", range(1, 16)), ("names", range(1, 16)), ("qualities", range(1, 16)),
                         ("bases", range(1, 16)), ("mixed", range(1, 16)), ("long", (1, 6, 15))):
        text, rec_off, want, want_off = expected[name]
        for shift in shifts:
            got, off, first_bad = from_fastq_dev(ctx, text, rec_off, in_shift=shift, out_shift=(5 * shift) % 16)
            assert (got, off, first_bad) == (want, want_off, len(rec_off) - 1), (name, shift)


def test_capacity_and_no_records(ctx, expected):
    text, rec_off, want, want_off = expected["names"]
    assert from_fastq_dev(ctx, text, rec_off, out_cap=len(want))[0] == want  # exactly enough
    for cap in (len(want) - 1, 32):
        with pytest.raises(api.FlxError) as e:
            from_fastq_dev(ctx, text, rec_off, out_cap=cap)
        assert e.value.code == 5 and e.value.needed == len(want)  # FLX_ERR_CAPACITY
        assert str(len(want)) in str(e.value)
    assert ctx.bam_from_fastq_dev(None, 0, None, 0, None, 0, None) == (0, 0)  # n_records == 0: a no-op
    assert api.bam_from_fastq(ctx, b"", [0]) == b""
    assert api.bam_from_fastq(ctx, text, rec_off, with_offsets=True) == (want, want_off)


def test_invalid_records_are_first_bad(ctx):
    for name, text, rec_off, want_bad in cases.damaged():
        assert from_fastq_dev(ctx, text, rec_off)[2] == want_bad, name
    # offsets that do not follow the records: first_bad, and (from_fastq_dev checks it) no write outside the buffers
    text, off = cases.text_of(cases.corpus()[0].entries[:6])
    shifted = list(off)
    shifted[3] += 1
    assert from_fastq_dev(ctx, text, shifted)[2] == 2
    past = list(off)
    past[-1] += 40
    assert from_fastq_dev(ctx, text, past)[2] == 5
    back = list(off)
    back[2] = off[1] - 1
    assert from_fastq_dev(ctx, text, back)[2] == 1
    overlap = [0] + [off[-1]] * 6  # every record but the first is empty, the first spans them all
    assert from_fastq_dev(ctx, text, overlap)[2] == 0
    with pytest.raises(ValueError):
        api.bam_from_fastq(ctx, text, shifted)


def walks_whole(z):
    in_off, out_off = api.bgzf_index(z)
    return int(in_off[-1]) == len(z)


def test_bgzf_bam_from_fastq(ctx, corpus, expected):
    names = [c.name for c in corpus]
    all_entries = [e for c in corpus for e in c.entries]
    text, rec_off = cases.text_of(all_entries)
    want = cases.expected_bam(all_entries)[0]
    longest = max(b - a for a, b in zip(rec_off, rec_off[1:]))
    # a slot above the text, slots below it (pieces of whole records), a slot below one record (the buffers grow)
    for slot_bytes in (16 << 20, 4 * 65280, 65280):
        assert slot_bytes == 16 << 20 or slot_bytes < len(text)
        z = api.Bgzf(ctx, slot_bytes=slot_bytes, slots=2)
        try:
            out = api.bgzf_bam_from_fastq(z, text, rec_off, eof=False)
            assert walks_whole(out) and gzip.decompress(out) == want, slot_bytes
            out = api.bgzf_bam_from_fastq(z, text, rec_off, eof=True)
            assert walks_whole(out) and out.endswith(_bam.EOF_BLOCK) and gzip.decompress(out) == want, slot_bytes
            assert api.bgzf_bam_from_fastq(z, b"", [0], eof=True) == _bam.EOF_BLOCK and api.bgzf_bam_from_fastq(z, b"", [0], eof=False) == b""
            with pytest.raises(ValueError):
                api.bgzf_bam_from_fastq(z, *cases.damaged()[0][1:3])
            with pytest.raises(api.FlxError) as e:
                api.bgzf_bam_from_fastq(z, text, rec_off, out_cap=100)
            assert e.value.code == 5
        finally:
            z.close()
    assert 65280 < longest
    # four threads at once on two slots: every call gives its own case's records
    z = api.Bgzf(ctx, slot_bytes=4 * 65280, slots=2)
    results = {}

    def work(name):
        results[name] = [api.bgzf_bam_from_fastq(z, expected[name][0], expected[name][1]) for _ in range(3)]
    try:
        threads = [threading.Thread(target=work, args=(n,)) for n in ("lengths", "names", "mixed", "long")]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
    finally:
        z.close()
    for name in ("lengths", "names", "mixed", "long"):
        assert len(results[name]) == 3 and all(gzip.decompress(o) == expected[name][2] and o.endswith(_bam.EOF_BLOCK) for o in results[name]), name
    assert set(names) >= set(results)
