"""The locus text itself (csrc/kmerset.h: flx_locus) — the words, the piece starts, U13, S1 and the seed table every refutation of
the cover kernels rests on — read back from finalized sets and checked against models written out here, for all three forms:
the assembly, the paths of the sequences' 24-mers (default for sets with short reads) and the paths of the members (order 16).
Membership comes from the oracle's set, never from the library.

tests/locus_text_peek.cpp is built here into a shared object that copies what flx_kmerset_locus() describes to the host.
With FLX_LOCUS_TEXT_RECORD=<file> every set's digests (text + safe1, the seed table as a sorted map) and the number of keys
the four-probe lookup of the kernels cannot reach are appended to that file, one JSON line per set."""
import ctypes as C
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import _cases
import _oracle
from filtlong_amd import _lib, api

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD, EMPTY, BACK_PAD = 2, 0xFFFFFFFF, 68  # kmerset.h: kLocusPad, kLocusEmpty; words of padding behind the data (at least)
SETS = ("assembly_a", "assembly_b", "order24", "order16", "tiny", "assembly_and_short")


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def peek_lib(tmp_path_factory, ctx):
    so = str(tmp_path_factory.mktemp("locus_text_peek") / "locus_text_peek.so")
    libdir = os.path.dirname(os.path.abspath(_lib.LIB_PATH))
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O1", "-std=c++17", "-shared", "-fPIC", "-I" + _lib.CSRC, "-o", so,
                           os.path.join(ROOT, "tests", "locus_text_peek.cpp"), "-L" + libdir, "-lfiltlong_hip", "-Wl,-rpath," + libdir])
    L = C.CDLL(so)
    L.locus_text_peek.argtypes = [C.c_void_p] * 5
    L.locus_text_peek.restype = C.c_int
    return L


def assembly_a():
    """Two add_assembly calls (two batches): contigs of 16, 15 (left out) and 45 bases, then one of 3000 with an N, a 40-base segment
    placed twice and the reverse complement of a 30-base stretch of itself.  n_text = 2 (16 + 45 + 3000) = 6122 = 16 * 382 + 10."""
    rng = np.random.RandomState(2024)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)

    def rnd(n):
        return acgt[rng.randint(0, 4, n)].tobytes()

    long_c = bytearray(rnd(3000))
    long_c[1500:1540] = long_c[500:540]
    long_c[2200:2230] = _cases.revcomp(bytes(long_c[800:830]))
    long_c[1000] = ord("N")
    return [[rnd(16), rnd(15), rnd(45)], [bytes(long_c)]]


def assembly_b():
    rng = np.random.RandomState(2025)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    return [[acgt[rng.randint(0, 4, n)].tobytes() for n in (16, 48)]]  # n_text = 128: the last data word is full


def kmers_at(codes):
    """the 16 codes from every position on as one number (first base on top); codes behind the end count as 0"""
    c = np.concatenate([codes.astype(np.uint32), np.zeros(16, dtype=np.uint32)])
    k = np.zeros(len(codes), dtype=np.uint32)
    for j in range(16):
        k |= c[j:j + len(codes)] << np.uint32(30 - 2 * j)
    return k


class Peek:
    """One finalized set: its oracle members, the arrays read back, and what every test derives from the TEXT WORDS alone."""

    def __init__(self, name, ctx, L, assembly_batches, short_files, env=None):
        self.name, self.contigs = name, [c for b in assembly_batches for c in b]
        orc = _oracle.KmerSet()
        orc.add_assembly(self.contigs)
        for f in short_files:
            orc.add_short_reads(f)
        self.members = np.sort(orc.dump())
        with pytest.MonkeyPatch.context() as mp:
            for k, v in (env or {}).items():
                mp.setenv(k, v)
            ks = api.Kmers(ctx)
            for b in assembly_batches:
                ks.add_assembly_fasta(b)
            ks.add_read_fastqs(short_files)
            ks.finalize()
        assert len(ks) == len(self.members)
        info = (C.c_uint64 * 6)()
        assert L.locus_text_peek(ks.h, info, None, None, None) == 0
        assert info[0] == 1 and info[5] == 1, "the set has no text, or no safe1"
        self.n_alloc, self.n_text, self.slots, self.shift = int(info[1]), int(info[2]), int(info[3]), int(info[4])
        self.text = np.zeros((self.n_alloc, 2), dtype=np.uint32)
        self.safe1 = np.zeros(self.n_alloc, dtype=np.uint16)
        self.seed = np.zeros(self.slots, dtype=np.uint32)
        assert L.locus_text_peek(ks.h, info, self.text.ctypes.data, self.safe1.ctypes.data, self.seed.ctypes.data) == 0
        ks.close()
        # ---- derived from the words ----
        self.n_words = (self.n_text + 15) // 16
        data = self.text[PAD:PAD + self.n_words]
        j = np.arange(16, dtype=np.uint32)
        self.codes = ((data[:, :1] >> (30 - 2 * j)) & 3).reshape(-1)[:self.n_text].astype(np.uint8)
        self.start = ((data[:, 1:] >> j) & 1).reshape(-1).astype(bool)  # every position of the data words, those behind n_text included
        self.starts = np.nonzero(self.start[:self.n_text])[0]
        ends = np.append(self.starts[1:], self.n_text)
        t = np.arange(self.n_text)
        assert self.start[0], "the text does not begin with a piece"
        self.piece_end = ends[np.searchsorted(self.starts, t, side="right") - 1]
        self.k16 = kmers_at(self.codes)

    def in_piece(self, length):
        return np.arange(self.n_text) + length <= self.piece_end

    def word_bits(self, per_position):
        """bit k of entry w = per_position[16 w + k], as the 16-bit fields of the data words hold them"""
        b = np.zeros(16 * self.n_words, dtype=np.uint32)
        b[:self.n_text] = per_position
        return (b.reshape(-1, 16) << np.arange(16, dtype=np.uint32)).sum(axis=1).astype(np.uint32)

    def seed_map(self):
        """(16-mer, position) of every occupied slot, and the slot's distance from its key's hash"""
        slot = np.nonzero(self.seed != EMPTY)[0]
        pos = self.seed[slot]
        assert (pos < self.n_text).all()
        key = self.k16[pos]
        h = ((key.astype(np.uint64) * 0x9E3779B1) & 0xFFFFFFFF) >> self.shift
        return key, pos, slot, (slot - h.astype(np.int64)) & (self.slots - 1), h.astype(np.int64)


@pytest.fixture(scope="module")
def peeks(ctx, peek_lib):
    """name -> Peek, each set built and read back once"""
    made = {}

    def get(name):
        if name not in made:
            case = _cases.path_text_case()
            args = {"assembly_a": (assembly_a(), []), "assembly_b": (assembly_b(), []), "order24": ([], case["files"]),
                    "order16": ([], case["files"], {"FLX_KMER_TEXT_ORDER": "16"}), "tiny": ([], [case["tiny"]]),
                    "assembly_and_short": ([[case["asm"]]], case["files"])}[name]
            made[name] = Peek(name, ctx, peek_lib, *args)
            record(made[name])
        return made[name]

    return get


@pytest.fixture
def pk(request, peeks):
    return peeks(request.param)


every_set = pytest.mark.parametrize("pk", SETS, indirect=True)
assemblies = pytest.mark.parametrize("pk", SETS[:2], indirect=True)
with_short_reads = pytest.mark.parametrize("pk", SETS[2:], indirect=True)


def record(p):
    key, pos, _slot, dist, _h = p.seed_map()
    order = np.lexsort((pos, key))
    line = {"set": p.name, "n_text": p.n_text, "members": len(p.members), "seed_keys": len(key),
            "text_safe1_sha256": hashlib.sha256(p.text.tobytes() + p.safe1.tobytes()).hexdigest(),
            "seed_map_sha256": hashlib.sha256(key[order].tobytes() + pos[order].tobytes()).hexdigest(),
            "keys_beyond_four_probes": int((dist >= 4).sum())}  # cover_common.h: the lookup tries slots hash .. hash + 3
    print(json.dumps(line))
    if os.environ.get("FLX_LOCUS_TEXT_RECORD"):
        with open(os.environ["FLX_LOCUS_TEXT_RECORD"], "a") as f:
            f.write(json.dumps(line) + "\n")


@every_set
def test_sizes_and_padding(pk):
    assert pk.n_text > 0 and pk.n_alloc >= pk.n_words + PAD + BACK_PAD
    pad = np.concatenate([pk.text[:PAD], pk.text[PAD + pk.n_words:]])
    assert (pad[:, 0] == 0).all() and ((pad[:, 1] & 0xFFFF) == 0xFFFF).all()
    assert pk.start[pk.n_text:].all(), "start bits behind n_text in the last data word"
    assert pk.start[0]
    if pk.name == "assembly_a":
        assert pk.n_text == 6122 and pk.n_text % 16
    if pk.name == "assembly_b":
        assert pk.n_text == 128


@every_set
def test_every_window_inside_a_piece_is_a_member(pk):
    assert (np.diff(np.append(pk.starts, pk.n_text)) >= 16).all()
    assert np.isin(pk.k16[pk.in_piece(16)], pk.members).all()


@assemblies
def test_assembly_text_is_both_strands_of_every_contig(pk):
    fwd, rev = np.zeros(256, dtype=np.uint8), np.zeros(256, dtype=np.uint8)
    for ch, f, r in ((b"Aa", 0, 3), (b"Cc", 1, 2), (b"Gg", 2, 1), (b"Tt", 3, 0)):  # anything else: 0 on both strands
        fwd[list(ch)], rev[list(ch)] = f, r
    codes, starts, at = [], [], 0
    for c in pk.contigs:
        if len(c) < 16:
            continue
        b = np.frombuffer(c, dtype=np.uint8)
        codes += [fwd[b], rev[b[::-1]]]
        starts += [at, at + len(b)]
        at += 2 * len(b)
    codes = np.concatenate(codes)
    assert pk.n_text == len(codes)
    assert (pk.codes == codes).all()
    assert (pk.starts == np.array(starts)).all()


@with_short_reads
def test_every_member_is_a_window(pk):
    windows = pk.k16[pk.in_piece(16)]
    assert np.isin(pk.members, windows).all()
    if pk.name == "order16":  # every member lies on exactly one path
        assert len(windows) == len(pk.members) == len(np.unique(windows))


@every_set
def test_u13_marks_the_13_windows_that_occur_once(pk):
    inside = pk.in_piece(13)
    v = pk.k16 >> 6
    vals, counts = np.unique(v[inside], return_counts=True)
    once = np.zeros(pk.n_text, dtype=bool)
    once[inside] = counts[np.searchsorted(vals, v[inside])] == 1
    want = np.zeros(pk.n_alloc, dtype=np.uint32)
    want[PAD:PAD + pk.n_words] = pk.word_bits(once)
    assert (pk.text[:, 1] >> 16 == want).all()
    assert once.any()


@every_set
def test_safe1_marks_the_windows_without_a_member_one_base_away(pk):
    inside = pk.in_piece(16)
    k = pk.k16[inside]
    near = np.zeros(len(k), dtype=bool)
    for j in range(16):
        for x in (1, 2, 3):
            nb = k ^ np.uint32(x << (2 * j))
            at = np.minimum(np.searchsorted(pk.members, nb), len(pk.members) - 1)
            near |= pk.members[at] == nb
    safe = np.zeros(pk.n_text, dtype=bool)
    safe[inside] = ~near
    want = np.zeros(pk.n_alloc, dtype=np.uint16)
    want[PAD:PAD + pk.n_words] = pk.word_bits(safe)
    assert (pk.safe1 == want).all()
    assert safe.any()


@every_set
def test_seed_table_maps_every_window_to_its_smallest_position(pk):
    assert pk.slots >= 1024 and pk.slots & (pk.slots - 1) == 0 and pk.shift == 32 - (pk.slots.bit_length() - 1)
    key, pos, slot, dist, h = pk.seed_map()
    t = np.nonzero(pk.in_piece(16))[0]
    want_key, first = np.unique(pk.k16[t], return_index=True)  # (t ascends: the first occurrence is the smallest position)
    order = np.argsort(key, kind="stable")
    assert len(key) == len(want_key) and (key[order] == want_key).all() and (pos[order] == t[first]).all()
    # reachable: no empty slot between the key's hash and its slot (linear probing, wrapping around)
    empties = np.concatenate([[0], np.cumsum(np.tile(pk.seed == EMPTY, 2))])
    assert (empties[h + dist + 1] - empties[h] == 0).all()
