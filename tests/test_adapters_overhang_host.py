"""The host walks of --adapter_overhang (csrc/adapters.h: end_key with both walks) without a GPU: tests/adapters_overhang_host.cpp runs
them as a stand-alone program, built with -O2 and again with the address and undefined-behaviour sanitizers (no preload, no Python, no
GPU; every read sits in a heap block of exactly its size).  Held, for equality, against tests/_adapters_overhang_model.py — the plain
dynamic programme, not the bit-vector form."""
import os
import struct
import subprocess

import numpy as np
import pytest

import _adapters_cases as cases
import _adapters_overhang_cases as ocases
import _adapters_overhang_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILDS = {"O2": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover"]}


@pytest.fixture(scope="module", params=sorted(BUILDS))
def program(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("adapters_overhang_" + request.param) / "adapters_overhang_host")
    subprocess.check_call(["g++", "-std=c++17"] + BUILDS[request.param] + ["-I" + os.path.join(ROOT, "filtlong_amd", "csrc"), "-o", exe,
                                                                          os.path.join(ROOT, "tests", "adapters_overhang_host.cpp")])
    return exe


def run(exe, tmp_path, seqs, errors, window, overhang, reads):
    """(build's answer, whether set_overhang took O, patterns [(m, k, o, k_o)], keys [n, 2])"""
    src, dst = str(tmp_path / "in"), str(tmp_path / "out")
    with open(src, "wb") as f:
        f.write(struct.pack("<iiiiQ", errors, window, overhang, 0, len(seqs)))
        for s in seqs:
            f.write(struct.pack("<Q", len(s)) + bytes(s))
        f.write(struct.pack("<Q", len(reads)))
        for r in reads:
            f.write(struct.pack("<Q", len(r)) + bytes(r))
    p = subprocess.run([exe, src, dst], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    blob = open(dst, "rb").read()
    rc, took = struct.unpack_from("<qq", blob, 0)
    if rc != 0 or not took:
        assert len(blob) == 16
        return rc, took, [], None
    n, = struct.unpack_from("<Q", blob, 16)
    pats = [struct.unpack_from("<IIII", blob, 24 + 16 * i) for i in range(n)]
    keys = np.frombuffer(blob, dtype=np.uint32, offset=24 + 16 * n).reshape(-1, 2)
    assert len(keys) == len(reads)
    return rc, took, pats, keys


WANT = {}


def same(got, want, reads):
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, [(int(i), len(reads[i]), got[i].tolist(), want[i].tolist()) for i in bad[:8]]


def test_allowances_and_range(program, tmp_path):
    rng = np.random.default_rng(5)
    seqs = [cases.random_adapter(rng, m) for m in (12, 13, 28, 32, 63, 64)]
    for overhang in (0, 1, 16, 52):
        for errors in (0, 20, 40):
            rc, took, pats, _ = run(program, tmp_path, seqs, errors, 150, overhang, [])
            assert rc == 0 and took and len(pats) == 2 * len(seqs)
            for (m, k, o, k_o), q in zip(pats, model.patterns(seqs)):
                assert (m, k, o, k_o) == (len(q), len(q) * errors // 100, model.overhang_of(len(q), overhang), model.edits_anchored(len(q), errors, overhang))
    for overhang in (-1, 53, 64, 1 << 20):
        assert run(program, tmp_path, seqs, 20, 150, overhang, [])[:2] == (0, 0)


@pytest.mark.parametrize("overhang,errors,window", [(8, 20, 150), (1, 40, 150), (11, 0, 12), (12, 20, 1), (51, 40, 40), (52, 20, 150), (16, 20, 1024)])
def test_keys(program, tmp_path, overhang, errors, window):
    rng = np.random.default_rng(100 * overhang + window)
    seqs = [cases.LIGATION, cases.random_adapter(rng, 12), cases.random_adapter(rng, 13), cases.random_adapter(rng, 64), cases.random_adapter(rng, 63),
            cases.random_adapter(rng, 32)]
    order = {150: (0, 3), 1024: (3,), 40: (4, 5)}.get(window, (2, 5))
    planted = [seqs[i] for i in order] + [s for i, s in enumerate(seqs) if i not in order]
    reads = ocases.reads_for(rng, planted, errors, window, overhang, planted=len(order))
    rc, took, _, got = run(program, tmp_path, planted, errors, window, overhang, reads)
    assert rc == 0 and took
    config = (overhang, errors, window)
    if config not in WANT:  # (both builds are held against one walk of the model)
        WANT[config] = model.keys_of(reads, window, model.patterns(planted), errors, overhang)
    same(got, WANT[config], reads)


def test_overhang_zero(program, tmp_path):
    """O = 0: the keys of --trim_adapters alone, and no pattern has a second walk"""
    rng = np.random.default_rng(2)
    seqs = [cases.LIGATION, cases.random_adapter(rng, 40)]
    reads = ocases.reads_for(rng, seqs, 20, 150, 8, planted=1)
    rc, took, pats, got = run(program, tmp_path, seqs, 20, 150, 0, reads)
    assert rc == 0 and took and all(p[2] == 0 for p in pats)
    import _adapters_model as plain
    same(got, plain.keys_of(reads, 150, model.patterns(seqs), 20), reads)


def test_every_overhang_of_one_pattern(program, tmp_path):
    """m = 64, every O from 1 to 52 (bit 63 of the first column, every shift), exact remnants at every truncation up to O + 2"""
    rng = np.random.default_rng(64)
    a = cases.random_adapter(rng, 64)
    pats = model.patterns([a])
    for overhang in (1, 2, 31, 32, 33, 51, 52):
        reads = []
        for x in range(0, min(overhang + 3, 64)):
            reads.append(a[x:] + cases.random_seq(rng, 90))
            reads.append(cases.random_seq(rng, 90) + a[:64 - x])
        rc, took, _, got = run(program, tmp_path, [a], 10, 100, overhang, reads)
        assert rc == 0 and took
        same(got, model.keys_of(reads, 100, pats, 10, overhang), reads)
