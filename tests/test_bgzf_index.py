"""flx_bgzf_index through ctypes, without a device: which members at the front of a buffer are BGZF members."""
import gzip
import struct

import numpy as np
import pytest

import _bgzf
import _bgzf_inflate_cases as cases
from filtlong_amd import _lib, api


@pytest.fixture(scope="module", autouse=True)
def library():
    import os
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()


@pytest.fixture(scope="module")
def members():
    return cases.small_members(9)


def offsets(ms):
    return ([0] + list(np.cumsum([len(m) for m, _ in ms])), [0] + list(np.cumsum([len(d) for _, d in ms])))


def index(data, **kw):
    a, b = api.bgzf_index(data, **kw)
    return [int(x) for x in a], [int(x) for x in b]


def test_a_bgzf_file(members):
    data = b"".join(m for m, _ in members) + _bgzf.EOF_BLOCK
    io, oo = offsets(members)
    assert index(data) == (io + [io[-1] + 28], oo + [oo[-1]])
    assert index(_bgzf.EOF_BLOCK) == ([0, 28], [0, 0])
    # what the index names is what the strict validator sees
    info = _bgzf.validate(data)[1]
    assert [(at, at + size) for at, size, _ in info["members"]] == list(zip(io + [io[-1]], io[1:] + [io[-1] + 28]))


def test_empty_and_short_inputs(members):
    assert index(b"") == ([0], [0])
    m = members[0][0]
    for n in (1, 17, 25, len(m) - 1):
        assert index(m[:n]) == ([0], [0])
    assert index(m) == ([0, len(m)], [0, len(members[0][1])])


def test_bgzf_then_plain_gzip(members):
    io, oo = offsets(members[:3])
    data = b"".join(m for m, _ in members[:3]) + gzip.compress(b"plain member") + members[3][0]
    assert index(data) == (io, oo)


def test_foreign_subfield_in_front_of_bc(members):
    m, d = members[1]
    extra = b"XY" + struct.pack("<H", 3) + b"abc" + b"BC" + struct.pack("<H", 2)
    size = len(m) + 7
    alt = m[:10] + struct.pack("<H", len(extra) + 2) + extra + struct.pack("<H", size - 1) + m[18:]
    assert len(alt) == size
    assert index(alt + members[2][0]) == ([0, size, size + len(members[2][0])], [0, len(d), len(d) + len(members[2][1])])
    # a BC subfield of another length is not the BGZF field
    bad = alt.replace(b"BC" + struct.pack("<H", 2), b"BC" + struct.pack("<H", 3))
    assert index(bad) == ([0], [0])
    # no extra field at all
    assert index(gzip.compress(b"x" * 100)) == ([0], [0])


def test_forged_bsize(members):
    io, oo = offsets(members[:2])
    m = bytearray(members[2][0])
    m[16:18] = struct.pack("<H", len(m) + 50)  # past the end of the input
    assert index(b"".join(x for x, _ in members[:2]) + bytes(m)) == (io, oo)
    m[16:18] = struct.pack("<H", 20)           # smaller than header + trailer
    assert index(b"".join(x for x, _ in members[:2]) + bytes(m)) == (io, oo)


def test_isize_beyond_64k(members):
    io, oo = offsets(members[:2])
    m = members[2][0][:-4] + struct.pack("<I", 65537)
    assert index(b"".join(x for x, _ in members[:2]) + m + members[3][0]) == (io, oo)
    m = members[2][0][:-4] + struct.pack("<I", 65536)  # the largest a member may claim
    got = index(b"".join(x for x, _ in members[:2]) + m)
    assert got[0] == io + [io[-1] + len(m)] and got[1] == oo + [oo[-1] + 65536]


def test_max_members(members):
    data = b"".join(m for m, _ in members)
    io, oo = offsets(members)
    for k in (0, 1, 5, 9, 20):
        assert index(data, max_members=k) == (io[:min(k, 9) + 1], oo[:min(k, 9) + 1])
