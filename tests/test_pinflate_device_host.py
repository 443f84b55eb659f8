"""The command line's parallel gzip reader with a device inflater plugged in, on the CPU: tests/pinflate_device_host.cpp gives
ParallelInflate a flx_bgzf_inflate made of the host walk of the kernel's phases and compares every byte and the way the stream ends
with the reader that has no such object — for good BGZF files and for damaged ones, where the device's first bad member goes to zlib."""
import gzip
import os
import re
import struct
import subprocess

import pytest

import _bgzf
import _cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = dict(os.environ, FLX_CLI_PINFLATE_MIN="1", FLX_CLI_PINFLATE_CHUNK="2000")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("pinflate_device") / "pinflate_device_host")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-pthread", "-I" + os.path.join(ROOT, "filtlong_amd", "csrc"),
                           "-I" + os.path.join(ROOT, "filtlong_amd", "cli"), "-o", out, os.path.join(ROOT, "tests", "pinflate_device_host.cpp"), "-lz"])
    return out


@pytest.fixture(scope="module")
def blob():
    return _bgzf.zlib_bgzf(_cases.c1_fastq_bytes(n=400), 6)


def check(exe, tmp_path, data):
    p = tmp_path / "in.gz"
    p.write_bytes(data)
    r = subprocess.run([exe, str(p)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=ENV)
    assert r.returncode == 0, (r.stdout.decode(), r.stderr.decode()[-500:])
    m = re.match(rb"same (\d+) error (\d) device (\d+)", r.stdout)
    return int(m.group(1)), int(m.group(2)), int(m.group(3))


def test_good_file(exe, tmp_path, blob):
    n_members = len(_bgzf.validate(blob)[1]["members"])
    size, error, device = check(exe, tmp_path, blob)
    assert size == len(_bgzf.validate(blob)[0]) and not error and device == n_members
    size, error, device = check(exe, tmp_path, blob[:-28])  # no end-of-file block
    assert not error and device == n_members - 1


@pytest.mark.parametrize("how", ["bit", "crc", "isize", "cut_in_member", "cut_at_boundary", "bsize", "plain_member_behind",
                                 "garbage_behind_eof", "first_member"])
def test_damaged_file(exe, tmp_path, blob, how):
    ms = _bgzf.validate(blob)[1]["members"]
    k = 0 if how == "first_member" else len(ms) // 2
    at, size, _ = ms[k]
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
    size, error, device = check(exe, tmp_path, bytes(b))
    assert device == (len(ms) if how == "garbage_behind_eof" else k)  # exactly the members in front of the damage
    if how in ("bit", "crc", "isize", "first_member"):
        assert error
