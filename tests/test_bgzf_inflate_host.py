"""The BGZF member decoder of bgzf_inflate_member.h without a GPU: tests/bgzf_inflate_host.cpp walks its phases on the host, built
with -O2 and again with the address and undefined-behaviour sanitizers (a stand-alone program: no preload, no Python, no GPU).  The
whole corpus of tests/_bgzf_inflate_cases.py passes in both; the sanitizer build is the proof of the bounds on damaged input."""
import os
import struct
import subprocess

import pytest

import _bgzf_inflate_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILDS = {"O2": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover"]}


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("inflate_corpus"))
    return cases.corpus(cases.build_host_encoder(d), d)


@pytest.fixture(scope="module", params=sorted(BUILDS))
def decoder(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("inflate_" + request.param) / "bgzf_inflate_host")
    subprocess.check_call(["g++", "-std=c++17"] + BUILDS[request.param] +
                          ["-I" + os.path.join(ROOT, "filtlong_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "bgzf_inflate_host.cpp")])
    return exe


def run(decoder, tmp_path, members):
    src, dst = str(tmp_path / "corpus"), str(tmp_path / "results")
    cases.write_corpus(src, members)
    p = subprocess.run([decoder, src, dst], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    return cases.read_results(dst)


def test_corpus(decoder, corpus, tmp_path):
    res = run(decoder, tmp_path, [c.member for c in corpus])
    cases.check_results(corpus, res)
    kinds = {k: sum(c.kind == k for c in corpus) for k in ("valid", "damaged", "fuzz")}
    assert kinds["valid"] >= 35 and kinds["damaged"] == 20 and kinds["fuzz"] == 300
    assert any(c.name.startswith("own_encoder") for c in corpus)
    # the fuzzed members are no formality: some are caught, and the statuses are of more than one kind
    fuzz = [st for c, (st, _) in zip(corpus, res) if c.kind == "fuzz"]
    assert sum(st != 0 for st in fuzz) >= 250 and len(set(fuzz)) >= 4


def test_damaged_members_name_their_fault(decoder, tmp_path):
    want = {"btype3": 2, "len_nlen": 3, "cl_oversubscribed": 5, "cl_incomplete": 5, "lit_oversubscribed": 8, "lit_incomplete": 8,
            "dist_oversubscribed": 9, "dist_incomplete": 9, "no_end_of_block": 7, "distance_too_far": 12, "match_past_isize": 13,
            "symbol_286": 10, "distance_symbol_30": 11, "unassigned_distance_code": 11, "match_without_distance_code": 11,
            "input_runs_out": 14, "ends_one_byte_early": 15,
            "isize_plus_1": 16, "isize_minus_1": 13, "crc_bit": 17}
    cs = cases.damaged_cases()
    res = run(decoder, tmp_path, [c.member for c in cs])
    assert {c.name: st for c, (st, _) in zip(cs, res)} == want


def test_frames_the_decoder_refuses(decoder, tmp_path):
    """what flx_bgzf_index would not have let through still gets a status and touches nothing: a short member, no magic, an ISIZE
    that is not the room it was given, an extra field that runs past the member"""
    m, d = cases.small_members(1)[0]
    long_extra = bytearray(m)
    long_extra[10:12] = b"\xff\xff"
    members = [m, m[:20], b"\x00" + m[1:], bytes(long_extra)]
    src, dst = str(tmp_path / "corpus"), str(tmp_path / "results")
    with open(src, "wb") as f:
        f.write(struct.pack("<I", len(members) + 1))
        for x in members:
            f.write(struct.pack("<II", len(x), len(d)) + x)
        f.write(struct.pack("<II", len(m), len(d) + 1) + m)  # the caller's room is not the member's ISIZE
    p = subprocess.run([decoder, src, dst], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    res = cases.read_results(dst)
    assert res[0] == (0, d)
    assert [st for st, _ in res[1:]] == [1, 1, 1, 1]
    assert all(got == b"\xab" * len(got) for _, got in res[1:])
