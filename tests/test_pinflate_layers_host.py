"""The layers of the command line's parallel gzip reader, each on its own and on the CPU: the hand-off queue
(cli/pinflate_queue.h), the gzip member framing (csrc/gzip_framing.h, shared with flx_bgzf_index), and a round whose allocation
fails (cli/pinflate_rounds.h: a round commits or never happened).  Stand-alone programs, built three ways: plain, with the
address + undefined-behaviour sanitizers, with the thread sanitizer; tests/pinflate_device_host.cpp runs its files the same three
ways."""
import concurrent.futures
import gzip
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

import _bgzf
import _cases
from test_cli_pinflate import bgzf, read_like_fastq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROGRAMS = ["pinflate_queue_host", "gzip_framing_host", "pinflate_alloc_host", "pinflate_device_host"]
BUILDS = {"plain": ["-O2"],
          "asan_ubsan": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"],
          "tsan": ["-O1", "-g", "-fsanitize=thread"]}
ENV = dict(os.environ, FLX_CLI_PINFLATE_MIN="1", FLX_CLI_PINFLATE_CHUNK="2000")
LIMIT = 120  # seconds: a case that hangs fails here


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("pinflate_layers")

    def compile_one(job):
        name, build = job
        out = str(d / (name + "." + build))
        subprocess.check_call(["g++", "-std=c++17", "-pthread"] + BUILDS[build] +
                              ["-I" + os.path.join(ROOT, "filtlong_amd", "csrc"), "-I" + os.path.join(ROOT, "filtlong_amd", "cli"),
                               "-o", out, os.path.join(ROOT, "tests", name + ".cpp"), "-lz"])
        return job, out

    with concurrent.futures.ThreadPoolExecutor(min(12, os.cpu_count() or 1)) as pool:
        return dict(pool.map(compile_one, [(n, b) for n in PROGRAMS for b in BUILDS if (n, b) != ("pinflate_device_host", "plain")]))  # (test_pinflate_device_host.py has that one)


def run(exe, name, build, *args):
    r = subprocess.run([exe[name, build]] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=ENV, timeout=LIMIT)
    assert r.returncode == 0, (name, build, args, r.stdout.decode()[-500:], r.stderr.decode()[-2000:])
    return r.stdout.decode()


# ---- a. the queue --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("build", list(BUILDS))
@pytest.mark.parametrize("case", ["flow", "stop_while_producer_waits", "stop_while_reader_waits", "unread_at_destruction"])
def test_queue(exe, case, build):
    assert run(exe, "pinflate_queue_host", build, case) == "ok %s\n" % case


# ---- b. the framing -------------------------------------------------------------------------------------------------------

def member(payload=b"framing\n!", flg=4, extra=None, name=b"", comment=b"", hcrc=False, bsize=None, isize=None):
    """one gzip member around a stored deflate block; extra: the whole extra field, with {B} for the two BSIZE bytes"""
    deflate = b"\x01" + struct.pack("<HH", len(payload), len(payload) ^ 0xffff) + payload
    head = b"\x1f\x8b\x08" + bytes([flg]) + b"\0\0\0\0\0\xff"
    if extra is None:
        extra = b"BC\x02\0{B}"
    if flg & 4:
        head += struct.pack("<H", len(extra.replace(b"{B}", b"..")))
    tail = (name + b"\0" if flg & 8 else b"") + (comment + b"\0" if flg & 16 else b"") + (b"\x12\x34" if hcrc else b"")
    total = len(head) + (len(extra.replace(b"{B}", b"..")) if flg & 4 else 0) + len(tail) + len(deflate) + 8
    if flg & 4:
        head += extra.replace(b"{B}", struct.pack("<H", (total if bsize is None else bsize) - 1))
    return head + tail + deflate + struct.pack("<II", zlib.crc32(payload), len(payload) if isize is None else isize)


def framing_table():
    """name -> (bytes, kind, header parses)"""
    t = {}
    m = member()
    assert len(m) == 40 and gzip.decompress(m) == b"framing\n!"
    t["bgzf"] = (m, "bgzf", True)
    t["bgzf_then_more"] = (m + m, "bgzf", True)
    t["plain"] = (member(flg=0), "other", True)
    t["gzip_module"] = (gzip.compress(bytes(range(256))), "other", True)
    t["whole_member_of_24_bytes"] = (gzip.compress(b"x" * 100), "other", False)  # (fewer than 26: zlib's)
    t["fname"] = (member(flg=8, name=b"reads.fastq"), "other", True)
    t["fcomment"] = (member(flg=16, comment=b"a comment"), "other", True)
    t["fhcrc"] = (member(flg=2, hcrc=True), "other", True)
    t["bgzf_with_name_comment_hcrc"] = (member(flg=4 | 8 | 16 | 2, name=b"n", comment=b"c", hcrc=True), "bgzf", True)
    t["fextra_without_bc"] = (member(extra=b"XY\x02\0ab"), "other", True)
    t["bc_behind_another_subfield"] = (member(extra=b"XY\x03\0abcBC\x02\0{B}"), "bgzf", True)
    t["bc_with_slen_3"] = (member(extra=b"BC\x03\0{B}z"), "other", True)
    t["bc_cut_by_xlen"] = (member(extra=b"XY\x01\0aBC\x02\0{B}")[:10] + struct.pack("<H", 10) + member(extra=b"XY\x01\0aBC\x02\0{B}")[12:], "other", True)
    x = bytearray(m); x[10:12] = struct.pack("<H", 1000); t["xlen_past_the_data"] = (bytes(x), "other", False)
    for bit in (0x20, 0x40, 0x80):
        x = bytearray(m); x[3] |= bit; t["reserved_flag_%02x" % bit] = (bytes(x), "other", False)
    x = bytearray(m); x[2] = 7; t["cm_7"] = (bytes(x), "other", False)
    t["bsize_below_header_and_trailer"] = (member(bsize=25) + m, "other", True)
    t["bsize_exactly_header_and_trailer"] = (member(bsize=26) + m, "forged", True)  # (its "ISIZE" is deflate data: far beyond 64 KiB)
    t["bsize_beyond_the_data"] = (member(bsize=41), "other", True)
    t["bsize_to_the_last_byte"] = (member(bsize=41) + b"\0", "bgzf", True)
    t["isize_65536"] = (member(isize=65536), "bgzf", True)
    t["isize_65537"] = (member(isize=65537), "forged", True)
    t["no_magic"] = (b"\x1f\x8a" + m[2:], "none", False)
    t["magic_alone"] = (b"\x1f\x8b", "other", False)
    return t


@pytest.mark.parametrize("build", list(BUILDS))
def test_framing_table(exe, tmp_path, build):
    table = framing_table()
    names = sorted(table)
    for n in names:
        (tmp_path / n).write_bytes(table[n][0])
    lines = run(exe, "gzip_framing_host", build, *[tmp_path / n for n in names]).splitlines()
    assert len(lines) == len(names)
    for n, line in zip(names, lines):
        data, kind, header = table[n]
        f = line.split()
        assert (int(f[0]), f[1], int(f[7])) == (len(data), kind, int(header)), (n, line)
        if kind in ("bgzf", "forged"):
            assert int(f[5]) == struct.unpack_from("<I", data, int(f[3]) - 4)[0] and int(f[3]) <= len(data), (n, line)
            assert int(f[3]) == int(f[11]) and int(f[9]) + 8 <= int(f[3]), (n, line)  # the member has room for its header and trailer
    got = {n: l.split() for n, l in zip(names, lines)}
    assert int(got["bgzf"][3]) == 40 and int(got["bgzf"][9]) == 18 and int(got["bgzf"][5]) == 9
    assert int(got["fname"][9]) == 10 + len(b"reads.fastq") + 1 and int(got["fcomment"][9]) == 10 + len(b"a comment") + 1
    assert int(got["fhcrc"][9]) == 12 and int(got["bgzf_with_name_comment_hcrc"][9]) == 18 + 2 + 2 + 2
    assert int(got["bc_behind_another_subfield"][9]) == 25 and int(got["bc_with_slen_3"][11]) == 0 and int(got["bc_cut_by_xlen"][11]) == 0


@pytest.mark.parametrize("build", list(BUILDS))
def test_framing_every_prefix_of_a_member(exe, tmp_path, build):
    """A 40-byte BGZF member cut at every length, each in a heap block of exactly that size (the sanitized build sees a read past the
    end): nothing without the magic, no header in fewer than 27 bytes (26 and more than a trailer behind the header), no BGZF member
    before the last byte is there.  The same for the member's end: no trailer that is not whole."""
    m = member()
    (tmp_path / "m").write_bytes(m)
    lines = run(exe, "gzip_framing_host", build, "--prefixes", tmp_path / "m").splitlines()
    assert len(lines) == 41
    for n, line in enumerate(lines):
        f = line.split()
        assert int(f[0]) == n and f[1] == ("none" if n < 2 else "other" if n < 40 else "bgzf") and int(f[7]) == (n >= 27) and int(f[13]) == (n >= 2), line
    both = m + member(flg=0)
    (tmp_path / "two").write_bytes(both)
    crc, isize = struct.unpack_from("<II", m, 32)
    lines = run(exe, "gzip_framing_host", build, "--end", 32, crc, isize, tmp_path / "two").splitlines()
    for n, line in zip(range(32, len(both) + 1), lines):
        assert line == "%d %s" % (n, "truncated next 0" if n < 40 else "last next 40" if n < 42 else "member_follows next 40"), line
    for wrong in ((crc ^ 1, isize), (crc, isize + 1)):
        lines = run(exe, "gzip_framing_host", build, "--end", 32, wrong[0], wrong[1], tmp_path / "two").splitlines()
        assert lines[7] == "39 truncated next 0" and lines[8] == "40 mismatch next 0" and lines[-1].split()[1] == "mismatch"


def test_flx_bgzf_index_agrees_with_the_framing():
    """the library's index takes a member exactly where the shared framing says BGZF (and counts on behind it)"""
    from filtlong_amd import _lib, api
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    for n, (data, kind, _) in sorted(framing_table().items()):
        a, b = api.bgzf_index(data)
        assert (len(a) >= 2) == (kind == "bgzf"), n
        if kind == "bgzf":
            size = struct.unpack_from("<H", data, data.index(b"BC\x02\0") + 4)[0] + 1
            assert (int(a[1]), int(b[1])) == (size, struct.unpack_from("<I", data, size - 4)[0]), n
    m = member()
    for n in range(41):
        assert len(api.bgzf_index(m[:n])[0]) == (2 if n == 40 else 1)


# ---- c. a failed allocation inside a round ----------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def text():
    return read_like_fastq(np.random.RandomState(17), 34, 5000)  # 314 KB


@pytest.mark.parametrize("build", list(BUILDS))
@pytest.mark.parametrize("form", ["plain", "bgzf", "plain_from_4_KiB"])
def test_failed_allocation_in_a_round(exe, tmp_path, text, form, build):
    """plain_from_4_KiB: allocations from 4 KiB fail, not from 64 KiB — the buffers of every round, so that rounds fail which did not
    begin the member (all buffers of 64 KiB are made in the first round, and used again)"""
    assert 250000 < len(text) < 400000
    # (BGZF: one round of four runs, each of five or six 16 KiB members: four buffers of at least 64 KiB)
    (tmp_path / "in.gz").write_bytes(bgzf(text, 16384) if form == "bgzf" else gzip.compress(text, 6, mtime=0))
    out = run(exe, "pinflate_alloc_host", build, tmp_path / "in.gz", 4, *([4096] if form == "plain_from_4_KiB" else [])).split()
    print(form, build, " ".join(out))
    assert out[0] == "ok" and int(out[6]) == len(text), out
    K, failed = int(out[2]), int(out[4])
    assert K >= (20 if form == "plain_from_4_KiB" else 4) and failed >= K // 2, out  # (a run can make fewer allocations than the clean one)


# ---- d. tests/pinflate_device_host.cpp, sanitized -------------------------------------------------------------------------

def device_files():
    blob = _bgzf.zlib_bgzf(_cases.c1_fastq_bytes(n=400), 6)
    ms = _bgzf.validate(blob)[1]["members"]
    at, size, _ = ms[len(ms) // 2]
    f = {"good": blob, "no_eof_block": blob[:-28], "plain_member": gzip.compress(_cases.c1_fastq_bytes(n=400), 6),
         "bgzf_then_plain": blob[:at] + gzip.compress(b"@x\nACGT\n+\n!!!!\n"),
         "cut_in_member": blob[:at + size // 2], "garbage_behind_eof": blob + b"\x1f\x8bgarbage behind the end-of-file block"}
    b = bytearray(blob); b[at + 18 + (size - 26) // 2] ^= 0x04; f["bit"] = bytes(b)
    b = bytearray(blob); b[at + size - 7] ^= 0x40; f["crc"] = bytes(b)
    b = bytearray(blob); b[at + size - 4:at + size] = struct.pack("<I", struct.unpack_from("<I", b, at + size - 4)[0] - 1); f["isize"] = bytes(b)
    b = bytearray(blob); b[at + 16:at + 18] = struct.pack("<H", 0xfff0); f["bsize"] = bytes(b)
    b = bytearray(blob); b[at + 16:at + 18] = struct.pack("<H", 20); f["bsize_below_header"] = bytes(b)
    return f


@pytest.fixture(scope="module")
def device_corpus():
    return device_files()


@pytest.mark.parametrize("build", ["asan_ubsan", "tsan"])
@pytest.mark.parametrize("name", ["good", "no_eof_block", "plain_member", "bgzf_then_plain", "cut_in_member", "garbage_behind_eof", "bit", "crc",
                                  "isize", "bsize", "bsize_below_header"])
def test_device_host_program_sanitized(exe, tmp_path, device_corpus, name, build):
    (tmp_path / name).write_bytes(device_corpus[name])
    out = run(exe, "pinflate_device_host", build, tmp_path / name)
    assert out.startswith("same "), (name, out)
    assert int(out.split()[3]) == (name in ("bit", "crc", "isize", "garbage_behind_eof")), (name, out)
