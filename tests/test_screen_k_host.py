"""The host core of --exclude_k (csrc/screen_hash.h) without a GPU: tests/screen_k_host.cpp runs it as a stand-alone program, built
with -O2 and again with the address and undefined-behaviour sanitizers (no preload, no Python, no GPU; sequences and tables sit in heap
blocks of exactly their size).  Held, for equality, against tests/_screen_k_model.py.  And the new argument errors of the command
line, in their order behind the existing ones, as far as it goes without a device."""
import os
import struct
import subprocess

import numpy as np
import pytest

import _screen_k_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILDS = {"O2": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover"]}
KS = (16, 17, 24, 31)
EMPTY = (1 << 64) - 1


@pytest.fixture(scope="module", params=sorted(BUILDS))
def program(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("screen_k_" + request.param) / "screen_k_host")
    subprocess.check_call(["g++", "-std=c++17"] + BUILDS[request.param] + ["-I" + os.path.join(ROOT, "filtlong_amd", "csrc"), "-o", exe,
                                                                          os.path.join(ROOT, "tests", "screen_k_host.cpp")])
    return exe


def keys(exe, tmp_path, seq, k):
    """[(valid, forward, reverse complement, canonical)] of every window"""
    src, dst = str(tmp_path / "seq"), str(tmp_path / "keys")
    open(src, "wb").write(bytes(seq))
    p = subprocess.run([exe, "keys", str(k), src, dst], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    blob = open(dst, "rb").read()
    assert len(blob) == 25 * model.windows(len(seq), k)
    return [struct.unpack_from("<BQQQ", blob, 25 * i) for i in range(len(blob) // 25)]


def code(kmer):
    c = 0
    for ch in kmer:
        c = (c << 2) | b"ACGT".index(ch)
    return c


@pytest.mark.parametrize("k", KS)
def test_random_windows(program, tmp_path, k):
    rng = np.random.default_rng(100 + k)
    seq = bytearray(model.random_seq(rng, 600))
    for at in rng.integers(0, 600, size=6):
        seq[at] = int(rng.choice([78, 110, 0, 255, 45]))
    for at in rng.integers(0, 600, size=150):
        seq[at] |= 0x20  # lower case is a base
    got = keys(program, tmp_path, seq, k)
    want_keys, want_valid = model.window_keys(seq, k)
    assert [g[0] for g in got] == [int(v) for v in want_valid] and 0 < sum(g[0] for g in got) < len(got)
    for i, (valid, fwd, rc, key) in enumerate(got):
        if valid:
            w = bytes(seq[i:i + k]).upper()
            assert fwd == code(w) and rc == code(model.revcomp(w)) and key == min(fwd, rc) == int(want_keys[i]) == model.key_of(w)
            assert key < 1 << (2 * k)


def test_hand_made_windows(program, tmp_path):
    for k in KS:
        # all T: the largest forward code; its reverse complement is all A, code 0
        (valid, fwd, rc, key), = keys(program, tmp_path, b"T" * k, k)
        assert (valid, fwd, rc, key) == (1, (1 << (2 * k)) - 1, 0, 0)
        (valid, fwd, rc, key), = keys(program, tmp_path, b"a" * k, k)
        assert (valid, fwd, rc, key) == (1, 0, (1 << (2 * k)) - 1, 0)
        # a K-mer and its reverse complement have one key
        w = (b"ACGGTCATTGCAGGCTTAACCGTAGGCATCA")[:k]
        a, = keys(program, tmp_path, w, k)
        b, = keys(program, tmp_path, model.revcomp(w), k)
        assert a[3] == b[3] and a[1] == b[2] and a[2] == b[1] and a[1] != a[2]
        # a byte outside ACGTacgt anywhere in the window
        for at in (0, k // 2, k - 1):
            bad = bytearray(w)
            bad[at] = ord("N")
            assert keys(program, tmp_path, bad, k) == [(0, 0, 0, 0)]
        assert keys(program, tmp_path, w[:k - 1], k) == []
    for k in (16, 24, 30):  # an even-K reverse-complement palindrome: the key is both codes
        half = (b"ACGGTCATTGCAGGC")[:k // 2]
        pal = half + model.revcomp(half)
        (valid, fwd, rc, key), = keys(program, tmp_path, pal, k)
        assert valid == 1 and fwd == rc == key == code(pal)
    assert (1 << 62) - 1 < EMPTY  # the largest key of all (all T at K = 31 is code 2^62 - 1, its key 0) is not the empty mark
    assert keys(program, tmp_path, b"T" * 31, 31)[0][1] == (1 << 62) - 1


def test_windows_of(program):
    for k in KS:
        for n in (0, 1, k - 1, k, k + 1, 1000, 2**31 - 1):
            assert subprocess.check_output([program, "windows", str(n), str(k)]).decode().strip() == str(model.windows(n, k)) == str(max(0, n - k + 1))


def table(exe, tmp_path, cap, ops):
    src, dst = str(tmp_path / "ops"), str(tmp_path / "table")
    with open(src, "wb") as f:
        f.write(struct.pack("<Q", len(ops)))
        for op, key in ops:
            f.write(op.encode() + struct.pack("<Q", key))
    p = subprocess.run([exe, "table", str(cap), src, dst], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    blob = open(dst, "rb").read()
    assert len(blob) == 8 * (len(ops) + cap)
    return list(struct.unpack_from("<%dq" % len(ops), blob, 0)), list(struct.unpack_from("<%dQ" % cap, blob, 8 * len(ops)))


def slot(exe, key, cap):
    return int(subprocess.check_output([exe, "slot", str(key), str(cap)]).decode())


def keys_of_slot(exe, cap, want_slot, count):
    found, key = [], 1
    while len(found) < count:
        if slot(exe, key, cap) == want_slot:
            found.append(key)
        key += 1
    return found


def test_table_of_16_slots(program, tmp_path):
    cap = 16
    # keys whose home is the last slot: the second wraps to slot 0, the third to slot 1
    last = keys_of_slot(program, cap, cap - 1, 3)
    ops = [("f", last[0]), ("i", last[0]), ("i", last[1]), ("i", last[0]), ("i", last[2]), ("f", last[0]), ("f", last[1]), ("f", last[2]), ("i", last[1])]
    res, tab = table(program, tmp_path, cap, ops)
    assert res == [cap, 1, 1, 0, 1, cap - 1, 0, 1, 0]
    assert tab[cap - 1] == last[0] and tab[0] == last[1] and tab[1] == last[2] and tab[2:cap - 1] == [EMPTY] * (cap - 3)
    # a model of the table in Python, on random keys with duplicates, until the table is full: a full probe chain
    rng = np.random.default_rng(77)
    pool = [int(x) for x in rng.integers(0, 1 << 62, size=24, dtype=np.uint64)]
    ops = [("i", pool[int(i)]) for i in rng.integers(0, 24, size=120)] + [("i", p) for p in pool] + [("f", p) for p in pool] + [("f", 12345)]
    res, tab = table(program, tmp_path, cap, ops)
    want_tab, want = [EMPTY] * cap, []
    for op, key in ops:
        s, answer = slot(program, key, cap), None
        for n in range(cap):
            at = (s + n) % cap
            if want_tab[at] == key:
                answer = 0 if op == "i" else at
                break
            if want_tab[at] == EMPTY:
                if op == "i":
                    want_tab[at] = key
                answer = 1 if op == "i" else cap
                break
        want.append(answer if answer is not None else (-1 if op == "i" else cap))
    assert res == want and tab == want_tab
    assert EMPTY not in tab and -1 in res  # the table filled up: a key it does not hold is looked for in all 16 slots and refused
    assert sorted(tab) == sorted(set(k for (op, k), r in zip(ops, res) if op == "i" and r == 1))


# ---- the command line's new argument errors, behind the existing ones ----
EXE = os.path.join(ROOT, "filtlong_amd", "bin", "filtlong")
FASTQ = os.path.join(ROOT, "tests", "golden", "ref_fixtures", "test_sort.fastq")
FASTA = os.path.join(ROOT, "tests", "golden", "ref_fixtures", "test_reference.fasta")
BAD_K = b"Error: the value for --exclude_k must be an integer between 16 and 31\n"
NEEDS_EXCLUDE = b"Error: --exclude_k needs --exclude\n"
ENV_ANSWER = b"Error: unknown environment variable FLX_CLI_NO_SUCH_SWITCH (the FLX_CLI_* switches are listed in README.md)\n"


@pytest.fixture(scope="module")
def exe():
    if not os.path.exists(EXE):
        import __graft_entry__
        __graft_entry__.build()
    return EXE


def refused(exe, message, *args):
    p = subprocess.run([exe] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    return p.returncode == 1 and p.stdout == b"" and p.stderr == message


def accepted(exe, *args):
    """the arguments pass: the run goes on to the environment check, which answers before any device is asked for"""
    p = subprocess.run([exe] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, FLX_CLI_NO_SUCH_SWITCH="1"))
    return p.returncode == 1 and p.stdout == b"" and p.stderr == ENV_ANSWER


@pytest.mark.parametrize("value", ["15", "32", "x", "-1", "24.5", "", "1e1", "0"])
def test_exclude_k_out_of_range(exe, value):
    assert refused(exe, BAD_K, "--exclude", FASTA, "--exclude_k", value, FASTQ)
    assert refused(exe, BAD_K, "--exclude_k", value, "--min_length", "5", FASTQ)  # the value before the missing --exclude


@pytest.mark.parametrize("value", ["16", "17", "24", "31", "031"])
def test_exclude_k_in_range(exe, value):
    assert accepted(exe, "--exclude", FASTA, "--exclude_k", value, FASTQ)
    assert refused(exe, NEEDS_EXCLUDE, "--exclude_k", value, "--min_length", "5", FASTQ)


def test_the_new_checks_come_last(exe, tmp_path):
    bad = ["--exclude_k", "99"]
    missing = str(tmp_path / "missing.fa")
    assert refused(exe, b"Error: flag 'exclude_k' requires an argument but received none\n", FASTQ, "--exclude", FASTA, "--exclude_k")
    assert refused(exe, b"Error: cannot find file: " + missing.encode() + b"\n", *bad, "--exclude", missing, FASTQ)
    assert refused(exe, b"Error: the value for --exclude_percent must be greater than 0 and at most 100\n", *bad, "--exclude", FASTA, "--exclude_percent", "0", FASTQ)
    assert refused(exe, b"Error: --exclude_percent needs --exclude\n", *bad, "--exclude_percent", "5", "--min_length", "5", FASTQ)
    assert refused(exe, b"Error: the value for --min_length must be a positive integer\n", *bad, "--exclude", FASTA, "--min_length", "0", FASTQ)
    assert refused(exe, b"Error: the value for --adapter_split_errors must be an integer between 0 and 40\n", *bad, "--exclude", FASTA,
                   "--adapter_split_errors", "99", FASTQ)
    assert refused(exe, b"Error: --split_adapters needs --trim_adapters\n", *bad, "--exclude", FASTA, "--split_adapters", FASTQ)
    assert refused(exe, b"Error: --adapter_split_errors needs --split_adapters\n", *bad, "--exclude", FASTA, "--adapter_split_errors", "10", FASTQ)
    assert refused(exe, b"Error: --adapter_split_errors needs --split_adapters\n", "--exclude_k", "24", "--adapter_split_errors", "10", "--min_length", "5", FASTQ)


def test_help_is_the_reference_menu(exe):
    p = subprocess.run([exe, "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0 and b"exclude" not in p.stderr and b"--min_window_q [float]" in p.stderr
