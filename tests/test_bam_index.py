"""flx_bam_index through ctypes, without a device: the record offsets, the counts and the end states (the data ends where a record
ends, inside a record, or at a record or header that is malformed)."""
import ctypes as C

import numpy as np
import pytest

import _bam
import _bam_cases as cases
from filtlong_amd import _lib, api


def test_offsets_of_the_corpus():
    for c in cases.corpus():
        if any(len(r["seq"]) > 10000 for r in c.records):
            continue
        off, end = api.bam_index(cases.case_bam(c))
        assert end == api.BAM_END and [int(x) for x in off] == _bam.record_offsets(c.records, **c.header), c.name


def test_end_states():
    recs = cases.three_records()
    good = _bam.bam_bytes(recs)
    offs = _bam.record_offsets(recs)
    assert api.BAM_END == _bam.END and api.BAM_TRUNCATED == _bam.TRUNCATED and api.BAM_MALFORMED == _bam.MALFORMED and api.BAM_HEADER == _bam.HEADER
    for cut in range(len(good) + 1):
        off, end = api.bam_index(good[:cut])
        whole = sum(1 for o in offs[1:] if o <= cut)
        if cut < offs[0]:
            assert (len(off) - 1, end) == (0, api.BAM_TRUNCATED), cut
        else:
            assert len(off) - 1 == whole and end == (api.BAM_END if cut in offs else api.BAM_TRUNCATED), cut
            assert [int(x) for x in off] == offs[:whole + 1]
    for name, blob in cases.damaged():
        if name.startswith("cut_"):
            continue
        want, want_end = _bam.walk_model(blob)
        off, end = api.bam_index(blob)
        assert (len(off) - 1, end) == (len(want), want_end), name
    bad = _bam.header_bytes() + _bam.record_bytes(recs[0]) + _bam.record_bytes(recs[1], l_read_name=0) + _bam.record_bytes(recs[2])
    off, end = api.bam_index(bad)
    assert end == api.BAM_MALFORMED and len(off) - 1 == 1  # "malformed at record 1"
    assert api.bam_index(b"BAM\2" + good[4:])[1] == api.BAM_HEADER
    assert api.bam_index(b"")[1] == api.BAM_TRUNCATED


def test_max_records_and_count_only():
    recs = cases.three_records()
    good = _bam.bam_bytes(recs)
    offs = _bam.record_offsets(recs)
    off, end = api.bam_index(good, max_records=2)
    assert [int(x) for x in off] == offs[:3] and end == api.BAM_MORE
    off, end = api.bam_index(good, max_records=3)
    assert [int(x) for x in off] == offs and end == api.BAM_END
    off, end = api.bam_index(good, max_records=0)
    assert [int(x) for x in off] == offs[:1] and end == api.BAM_MORE
    L = _lib.load()
    src = np.frombuffer(good, dtype=np.uint8)
    n, e = C.c_uint64(), C.c_int()
    assert L.flx_bam_index(src.ctypes.data, len(src), 2 ** 64 - 1, None, C.byref(n), C.byref(e)) == 0  # rec_off NULL: count only
    assert (n.value, e.value) == (3, api.BAM_END)
    assert L.flx_bam_index(src.ctypes.data, len(src), 10, None, None, C.byref(e)) == 1  # FLX_ERR_INVALID
