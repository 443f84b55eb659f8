"""BGZF without a GPU: the validator of tests/_bgzf.py, and the member encoder of bgzf_member.h compiled for the host."""
import os
import random
import struct
import subprocess
import sys
import zlib

import pytest

import _bgzf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_fastq_ont  # noqa: E402


def test_validator_accepts_zlib_bgzf():
    data = bytes(random.Random(5).getrandbits(8) for _ in range(70000)) + b"ACGT" * 50000
    for level in (1, 6):
        s = _bgzf.zlib_bgzf(data, level)
        got, info = _bgzf.validate(s)
        assert got == data and info["eof"] and len(info["members"]) == 6
        assert [m[2] for m in info["members"]] == [65280] * 4 + [8880, 0]
    assert _bgzf.validate(_bgzf.EOF_BLOCK)[0] == b""
    assert _bgzf.validate(b"", require_eof=False)[0] == b""


@pytest.mark.parametrize("at,what", [(0, "ID1"), (1, "ID2"), (2, "CM"), (3, "FLG"), (10, "XLEN"), (12, "SI1"), (13, "SI2"),
                                     (14, "SLEN"), (16, "BSIZE"), (17, "BSIZE high"), (20, "deflate data"),
                                     (-8, "CRC-32"), (-5, "CRC-32 high"), (-4, "ISIZE"), (-1, "ISIZE high")])
def test_validator_rejects_one_corrupted_byte(at, what):
    data = b"@read\nACGTTGCA\n+\n!!!!####\n" * 200
    s = bytearray(_bgzf.zlib_bgzf(data, 6, eof=False))
    assert _bgzf.validate(bytes(s), require_eof=False)[0] == data
    s[at % len(s)] ^= 0x21
    with pytest.raises(_bgzf.BgzfError):
        _bgzf.validate(bytes(s), require_eof=False)


def test_validator_checks_the_eof_block():
    data = b"x" * 1000
    s = _bgzf.zlib_bgzf(data, 1, eof=False)
    with pytest.raises(_bgzf.BgzfError):
        _bgzf.validate(s)
    for k in range(len(_bgzf.EOF_BLOCK)):
        bad = bytearray(_bgzf.EOF_BLOCK)
        bad[k] ^= 0x01
        with pytest.raises(_bgzf.BgzfError):
            _bgzf.validate(s + bytes(bad))
    with pytest.raises(_bgzf.BgzfError):  # an empty member that is not the last
        _bgzf.validate(_bgzf.EOF_BLOCK + s + _bgzf.EOF_BLOCK)
    with pytest.raises(_bgzf.BgzfError):  # a member of more than 65536 bytes
        c = zlib.compressobj(0, zlib.DEFLATED, -15)
        body = c.compress(bytes(70000)) + c.flush()
        _bgzf.validate(_bgzf.HEADER + struct.pack("<H", 0) + body, require_eof=False)


@pytest.fixture(scope="module")
def host_encoder(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("bgzf") / "bgzf_host")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "filtlong_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "bgzf_host.cpp")])
    return exe


def host_bgzf(exe, tmp_path, data):
    src, dst = tmp_path / "in", tmp_path / "out"
    src.write_bytes(data)
    subprocess.check_call([exe, str(src), str(dst)])
    return dst.read_bytes()


def cases():
    r = random.Random(11)
    fib = [1, 1]
    while len(fib) < 25:
        fib.append(fib[-1] + fib[-2])
    skew = [i for i, f in enumerate(fib) for _ in range(min(f, 30000))]
    r.shuffle(skew)
    periodic = {p: (bytes(r.getrandbits(8) for _ in range(p)) * (140000 // p + 2))[:140000] for p in (1, 3, 257, 32768, 32769, 40000)}
    return [("one", b"Q"), ("all256", bytes(range(256))), ("random", bytes(r.getrandbits(8) for _ in range(140000))),
            ("run258", b"z" * 258), ("run", b"z" * 200000), ("fibonacci", bytes(skew))] + \
        [("period%d" % p, d) for p, d in periodic.items()] + [("ont", gen_fastq_ont.generate(400000, seed=3))]


@pytest.mark.parametrize("name,data", cases(), ids=[c[0] for c in cases()])
def test_host_encoder_round_trips(host_encoder, tmp_path, name, data):
    s = host_bgzf(host_encoder, tmp_path, data)
    got, info = _bgzf.validate(s)
    assert got == data
    for _, size, isize in info["members"][:-1]:
        assert size <= isize + 5 + 26  # never more than a stored block
    if name == "ont":
        assert len(s) <= 1.10 * len(_bgzf.zlib_bgzf(data, 1))


# ---- the command line's --gzip, where no GPU is involved ------------------------------------------------------------------------
BIN = os.path.join(ROOT, "filtlong_amd", "bin", "filtlong")


def run_cli(args):
    import _cases
    args = [os.path.join(_cases.FIXTURES, "test_sort.fastq") if a == "INPUT" else a for a in args]
    p = subprocess.run([BIN] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, LANG="C", LC_ALL="C"))
    return p.returncode, p.stdout, p.stderr


def test_gzip_version():
    rc, out, err = run_cli(["--gzip", "--version"])
    assert (rc, out, err) == (0, b"Filtlong v0.3.1\n", b"")


def test_argument_errors_are_the_same_with_gzip():
    import json
    cases = json.load(open(os.path.join(ROOT, "tests", "golden", "arg_errors.json")))
    for c in cases:
        argv = c["argv"]
        if "--gpus" in argv or any(a.startswith("-h") or a == "--help" for a in argv):
            continue
        plain = run_cli(argv)
        gz = run_cli(["--gzip"] + argv)  # (in front: behind a flag that wants a value it would be that value)
        assert gz[0] == plain[0] and gz[2] == plain[2], (argv, gz, plain)
        if plain[0] != 0:
            assert gz[1] == plain[1] == b""
