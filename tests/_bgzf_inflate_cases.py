"""The corpus of BGZF members for the inflate tests (host walk and GPU): members made by Python's zlib (wbits=-15, framed with
the header of tests/_bgzf.py) and members packed by hand for what zlib will not emit.

corpus(host_encoder=None) -> list of Case(name, member, data, kind):
  kind "valid":    the decoder must say 0 and give `data`;
  kind "damaged":  the decoder must give a status other than 0 (zlib_ok(member) is False for every one of them: checked here);
  kind "fuzz":     one random bit of a valid member's deflate data flipped — only "decoder ok => zlib ok with the same bytes".

Two cases of the issue's list cannot be framed as a BGZF member, whose BSIZE field ends at 65536 bytes: 65536 bytes in stored blocks
of 65535 + 1 (65572 bytes with the frame) and 64 KiB of random bytes (stored by zlib: 65567).  They are here at the largest size
that fits: stored blocks of 65499 + 1 bytes, and 65280 random bytes (bgzip's block size).  zlib never emits a distance beyond
32768 - 262, so the distance of exactly 32768 is packed by hand.
"""
import collections
import os
import random
import struct
import subprocess
import sys
import zlib

import _bgzf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_fastq_ont  # noqa: E402

Case = collections.namedtuple("Case", "name member data kind")


def frame(body, data=None, crc=None, isize=None):
    """header + BSIZE + deflate bytes + CRC-32 + ISIZE"""
    crc = zlib.crc32(data) if crc is None else crc
    isize = len(data) if isize is None else isize
    size = 18 + len(body) + 8
    assert size <= 65536, size
    return _bgzf.HEADER + struct.pack("<H", size - 1) + bytes(body) + struct.pack("<II", crc & 0xffffffff, isize & 0xffffffff)


def deflate(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    return c.compress(data) + c.flush()


def zlib_ok(member, want=None):
    """What the command line's reader asks of zlib for one member: the stream ends exactly at the trailer, ISIZE and CRC-32 hold."""
    body, (crc, isize) = member[18:-8], struct.unpack("<II", member[-8:])
    d = zlib.decompressobj(-15)
    try:
        data = d.decompress(body)
    except zlib.error:
        return False
    if not d.eof or d.unused_data or len(data) != isize or zlib.crc32(data) != crc:
        return False
    return want is None or data == want


# ---- packing deflate by hand ------------------------------------------------------------------------------------------------------
class Bits:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, v, n):  # n bits of v, least significant first
        self.acc |= (v & ((1 << n) - 1)) << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 0xff)
            self.acc >>= 8
            self.n -= 8

    def code(self, c, n):  # a Huffman code: most significant bit first
        for b in range(n - 1, -1, -1):
            self.put((c >> b) & 1, 1)

    def align(self):
        if self.n:
            self.put(0, 8 - self.n)

    def raw(self, data):
        assert self.n == 0
        self.out += data

    def bytes(self):
        self.align()
        return bytes(self.out)


def len_sym(L):
    if L == 258:
        return 285, 0, 0
    v = L - 3
    ne = 0 if v < 8 else v.bit_length() - 3
    return 257 + 4 * ne + (v >> ne), ne, v & ((1 << ne) - 1)


def dist_sym(D):
    d = D - 1
    ne = 0 if d < 2 else d.bit_length() - 2
    return 2 * ne + (d >> ne), ne, d & ((1 << ne) - 1)


def canonical(lens):
    """{symbol: (code, length)} of a list of code lengths (RFC 1951 3.2.2)"""
    count = [0] * 16
    for v in lens:
        count[v] += 1
    count[0] = 0
    nxt, c = [0] * 16, 0
    for k in range(1, 16):
        c = (c + count[k - 1]) << 1
        nxt[k] = c
    codes = {}
    for s, v in enumerate(lens):
        if v:
            codes[s] = (nxt[v], v)
            nxt[v] += 1
    return codes


FIXED_LIT = canonical([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8)
FIXED_DIST = canonical([5] * 32)
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
CL_LENS = [4] * 13 + [5] * 6  # a complete code-length code: 13/16 + 6/32


def tokens(bw, toks, lit, dist):
    """toks: ints (literals), (length, distance) pairs, ("sym", s) / ("dsym", length, d) for raw symbols; ends with 256"""
    for t in toks:
        if isinstance(t, int):
            bw.code(*lit[t])
        elif t[0] == "sym":
            bw.code(*lit[t[1]])
        elif t[0] == "dsym":
            s, ne, ev = len_sym(t[1])
            bw.code(*lit[s])
            bw.put(ev, ne)
            bw.code(*dist[t[2]])
        else:
            s, ne, ev = len_sym(t[0])
            bw.code(*lit[s])
            bw.put(ev, ne)
            s, ne, ev = dist_sym(t[1])
            bw.code(*dist[s])
            bw.put(ev, ne)
    bw.code(*lit[256])


def fixed_block(bw, toks, final=True):
    bw.put(1 if final else 0, 1)
    bw.put(1, 2)
    tokens(bw, toks, FIXED_LIT, FIXED_DIST)


def stored_block(bw, data, final=True, nlen=None):
    bw.put(1 if final else 0, 1)
    bw.put(0, 2)
    bw.align()
    bw.put(len(data), 16)
    bw.put((~len(data) & 0xffff) if nlen is None else nlen, 16)
    bw.raw(data)


def dynamic_header(bw, litlens, distlens, final=True, cl_lens=CL_LENS, hclen=19):
    """BFINAL, BTYPE 2, the counts, the code-length code, and litlens + distlens run-length coded as ONE sequence (so a run crosses
    from the literal/length lengths into the distance lengths wherever the values allow it)"""
    bw.put(1 if final else 0, 1)
    bw.put(2, 2)
    bw.put(len(litlens) - 257, 5)
    bw.put(len(distlens) - 1, 5)
    bw.put(hclen - 4, 4)
    for k in range(hclen):
        bw.put(cl_lens[CL_ORDER[k]], 3)
    cl = canonical(cl_lens)
    seq, i, runs = list(litlens) + list(distlens), 0, []
    while i < len(seq):
        v, r = seq[i], 1
        while i + r < len(seq) and seq[i + r] == v:
            r += 1
        if v == 0 and r >= 3:
            k = min(r, 138)
            runs.append((18, k - 11, 7) if k >= 11 else (17, k - 3, 3))
            i += k
        elif v != 0 and r >= 4:
            k = min(r - 1, 6)
            runs += [(v, 0, 0), (16, k - 3, 2)]
            i += 1 + k
        else:
            runs.append((v, 0, 0))
            i += 1
    for s, ev, ne in runs:
        if s in cl:
            bw.code(*cl[s])
        bw.put(ev, ne)
    return runs


def sparse(n, d):
    lens = [0] * n
    for s, v in d.items():
        lens[s] = v
    return lens


def dynamic_member(litlens, distlens, toks, data):
    bw = Bits()
    dynamic_header(bw, litlens, distlens)
    tokens(bw, toks, canonical(litlens), canonical(distlens))
    return frame(bw.bytes(), data)


def fib_bytes(nsym, seed):
    fib = [1, 1]
    while len(fib) < nsym:
        fib.append(fib[-1] + fib[-2])
    b = [i for i, f in enumerate(fib) for _ in range(f)]
    random.Random(seed).shuffle(b)
    return bytes(b)


def no_repeat_bytes():
    """259 bytes over 4 symbols in which no 4 bytes occur twice: the de Bruijn sequence B(4, 4) with its first 3 bytes behind it"""
    k, n, a, seq = 4, 4, [0] * 16, []

    def db(t, p):
        if t > n:
            if n % p == 0:
                seq.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, k):
                a[t] = j
                db(t + 1, t)

    db(1, 1)
    b = bytes(b"ACGT"[v] for v in seq + seq[:3])
    assert len(b) == 259 and len({b[i:i + 4] for i in range(256)}) == 256
    return b


def hdist_of(member):
    """HDIST + 1 of a member whose deflate data begins with a dynamic block"""
    v = int.from_bytes(member[18:21], "little")
    return (v >> 8 & 31) + 1


def own_encoder_members(exe, tmpdir, data):
    """the members tests/bgzf_host.cpp (the repository's encoder on the CPU) writes for `data`, without the end-of-file block"""
    src, dst = os.path.join(tmpdir, "enc_in"), os.path.join(tmpdir, "enc_out")
    open(src, "wb").write(data)
    subprocess.check_call([exe, src, dst])
    s = open(dst, "rb").read()
    got, info = _bgzf.validate(s)
    assert got == data
    out, pos = [], 0
    for at, size, isize in info["members"]:
        if isize:
            out.append((s[at:at + size], data[pos:pos + isize]))
        pos += isize
    return out


def build_host_encoder(tmpdir):
    exe = os.path.join(str(tmpdir), "bgzf_host")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "filtlong_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "bgzf_host.cpp")])
    return exe


def valid_cases(host_encoder=None, tmpdir=None):
    r = random.Random(41)
    ont = gen_fastq_ont.generate(200000, seed=5)
    rnd = bytes(r.getrandbits(8) for _ in range(65280))
    cs = [("eof", _bgzf.EOF_BLOCK, b"")]

    def z(name, data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
        cs.append((name, frame(deflate(data, level, strategy), data), data))

    z("isize1", b"A")
    z("isize65280", ont[:65280])
    z("isize65536", ont[:65536])
    bw = Bits()
    stored_block(bw, b"")
    cs.append(("stored_len0", frame(bw.bytes(), b""), b""))
    bw = Bits()
    stored_block(bw, rnd[:65499], final=False)
    stored_block(bw, rnd[65499:65500])
    cs.append(("stored_65499_plus_1", frame(bw.bytes(), rnd[:65500]), rnd[:65500]))
    z("z_fixed", ont[:30000], 6, zlib.Z_FIXED)
    for level in (0, 1, 6, 9):
        z("level%d" % level, ont[1000:1000 + 65280], level)
    # several blocks of all three types; the flushes leave empty stored blocks at odd bit offsets
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    parts = [ont[:20001], b"ab", rnd[:9000], ont[20001:33000], b"q"]
    body = c.compress(parts[0]) + c.flush(zlib.Z_FULL_FLUSH) + c.compress(parts[1]) + c.flush(zlib.Z_SYNC_FLUSH) + \
        c.compress(parts[2]) + c.flush(zlib.Z_SYNC_FLUSH) + c.compress(parts[3]) + c.flush(zlib.Z_FULL_FLUSH) + \
        c.compress(parts[4]) + c.flush()
    cs.append(("mixed_blocks", frame(body, b"".join(parts)), b"".join(parts)))
    bw = Bits()  # the same by hand: fixed, stored, dynamic, an empty stored block, fixed
    fixed_block(bw, list(b"hello ") + [(5, 6), (258, 1)], final=False)
    stored_block(bw, b"STORED", final=False)
    dynamic_header(bw, sparse(258, {65: 1, 256: 2, 257: 2}), [1, 1], final=False)
    tokens(bw, [65, 65, (3, 1), (3, 2)], canonical(sparse(258, {65: 1, 256: 2, 257: 2})), canonical([1, 1]))
    stored_block(bw, b"", final=False)
    fixed_block(bw, [(4, 8), 33])
    data = b"hello hello" + b"o" * 258 + b"STORED" + b"A" * 8
    data = data + data[-8:-4] + b"!"
    assert zlib.decompress(bw.bytes(), -15) == data
    cs.append(("mixed_by_hand", frame(bw.bytes(), data), data))
    for n in (3, 258, 259, 65536):
        z("run%d" % n, b"\xee" * n)
    for p in (2, 3, 257):
        base = bytes(r.getrandbits(8) for _ in range(p))
        z("period%d" % p, (base * (65536 // p + 1))[:65536], 9)
    base = bytes(r.getrandbits(8) for _ in range(32768))
    z("period32000_zlib", base[:32000] * 2, 9)  # (the farthest period zlib still finds: its window ends 262 short of 32768)
    bw = Bits()  # distance exactly 32768; the first match's source starts at output byte 0
    stored_block(bw, base, final=False)
    fixed_block(bw, [(258, 32768)] * 126 + [(257, 32768), (3, 32768)])
    cs.append(("period32768_by_hand", frame(bw.bytes(), base * 2), base * 2))
    z("random65280", rnd)
    z("all256", bytes(range(256)))
    z("all256_l9", bytes(range(256)), 9)
    fib = fib_bytes(21, 1)  # 28656 bytes, 21 symbols: the unlimited code would be 20 bits deep, zlib limits it to 15
    z("fibonacci", fib)
    z("fibonacci_huffman_only", fib, 6, zlib.Z_HUFFMAN_ONLY)
    # code-length runs across the HLIT / HDIST boundary: 12 + 4 zeros as one symbol 18; five 2s behind a 2 as one symbol 16
    lit = sparse(270, {65: 1, 256: 2, 257: 2})
    dist = [0, 0, 0, 0, 1]
    bw = Bits()
    runs = dynamic_header(bw, lit, dist)
    assert (18, 16 - 11, 7) in runs
    tokens(bw, [65] * 8 + [(3, 5)], canonical(lit), canonical(dist))
    cs.append(("cl_zero_run_crosses", frame(bw.bytes(), b"A" * 11), b"A" * 11))
    lit = sparse(258, {65: 1, 256: 2, 257: 2})
    dist = [2, 2, 2, 2]
    bw = Bits()
    runs = dynamic_header(bw, lit, dist)
    assert runs[-2:] == [(2, 0, 0), (16, 5 - 3, 2)]
    tokens(bw, [65] * 4 + [(3, 1), (3, 4)], canonical(lit), canonical(dist))
    cs.append(("cl_repeat_crosses", frame(bw.bytes(), b"A" * 10), b"A" * 10))
    # literals only in a dynamic block whose distance set is empty (HDIST 1, the one length 0): zlib's build_tree never writes this
    # (it forces two distance codes, and stores bytes(range(256))), this repository's encoder does for a member without a match
    lit = sparse(257, {65: 2, 66: 2, 67: 2, 256: 2})
    bw = Bits()
    dynamic_header(bw, lit, [0])
    tokens(bw, list(b"ABCCBA"), canonical(lit), {})
    cs.append(("literal_only_no_distance_code", frame(bw.bytes(), b"ABCCBA"), b"ABCCBA"))
    if host_encoder:
        for k, (m, d) in enumerate(own_encoder_members(host_encoder, tmpdir, ont[:150000] + rnd[:3000] + b"\xee" * 70000 + fib)):
            cs.append(("own_encoder_%d" % k, m, d))
        # no match for the encoder (every 4 bytes occur once) and few enough symbols that the dynamic block beats the stored one
        (m, d), = own_encoder_members(host_encoder, tmpdir, no_repeat_bytes())
        assert (m[18] >> 1) & 3 == 2 and hdist_of(m) == 1, "a dynamic block with HDIST 1"
        cs.append(("own_encoder_no_match", m, d))
    out = [Case(n, m, d, "valid") for n, m, d in cs]
    for c in out:
        assert zlib_ok(c.member, c.data), c.name
    return out


def damaged_cases():
    ont = gen_fastq_ont.generate(70000, seed=6)
    good = deflate(ont[:40000])
    data = ont[:40000]
    cs = []
    cs.append(("btype3", frame(b"\x07\x00\x00\x00\x00", b"")))
    bw = Bits()
    stored_block(bw, b"12345", nlen=0)
    cs.append(("len_nlen", frame(bw.bytes(), b"12345")))

    def header_only(name, litlens, distlens, **kw):
        bw = Bits()
        dynamic_header(bw, litlens, distlens, **kw)
        bw.put(0, 64)
        cs.append((name, frame(bw.bytes(), b"")))

    ok_lit = sparse(258, {65: 1, 256: 2, 257: 2})
    header_only("cl_oversubscribed", ok_lit, [1, 1], cl_lens=[4] * 19)
    header_only("cl_incomplete", ok_lit, [1, 1], cl_lens=sparse(19, {0: 2, 1: 2, 2: 2}))
    header_only("lit_oversubscribed", sparse(258, {0: 1, 1: 1, 2: 1, 256: 2}), [1, 1])
    header_only("lit_incomplete", sparse(258, {65: 2, 256: 2}), [1, 1])
    header_only("dist_oversubscribed", ok_lit, [1, 1, 1])
    header_only("dist_incomplete", ok_lit, [2, 2])
    header_only("no_end_of_block", sparse(257, {65: 1, 66: 1}), [1, 1])
    bw = Bits()
    fixed_block(bw, [65, (3, 2)])
    cs.append(("distance_too_far", frame(bw.bytes(), b"AAAA")))
    bw = Bits()
    fixed_block(bw, [65, (10, 1)])
    cs.append(("match_past_isize", frame(bw.bytes(), b"AAAAA")))
    bw = Bits()
    fixed_block(bw, [65, ("sym", 286)])
    cs.append(("symbol_286", frame(bw.bytes(), b"A")))
    bw = Bits()
    fixed_block(bw, [65, ("dsym", 3, 30)])
    cs.append(("distance_symbol_30", frame(bw.bytes(), b"AAAA")))
    bw = Bits()  # a single distance code of one bit (allowed), and the block uses the other bit
    lit, dist = ok_lit, [1]
    dynamic_header(bw, lit, dist)
    bw.code(*canonical(lit)[65])
    bw.code(*canonical(lit)[257])
    bw.put(1, 1)
    bw.put(0, 16)
    cs.append(("unassigned_distance_code", frame(bw.bytes(), b"AAAA")))
    bw = Bits()  # no distance code at all (allowed in a block without a match), and the block has a match
    lit = sparse(258, {65: 1, 256: 2, 257: 2})
    dynamic_header(bw, lit, [0])
    bw.code(*canonical(lit)[65])
    bw.code(*canonical(lit)[257])
    bw.put(0, 16)
    cs.append(("match_without_distance_code", frame(bw.bytes(), b"AAAA")))
    cs.append(("input_runs_out", frame(good[:-3], data)))
    cs.append(("ends_one_byte_early", frame(good + b"\x00", data)))
    cs.append(("isize_plus_1", frame(good, data, isize=len(data) + 1)))
    cs.append(("isize_minus_1", frame(good, data, isize=len(data) - 1)))
    cs.append(("crc_bit", frame(good, data, crc=zlib.crc32(data) ^ 0x00010000)))
    out = [Case(n, m, None, "damaged") for n, m in cs]
    for c in out:
        assert not zlib_ok(c.member), c.name
    return out


def fuzz_cases(n=300, seed=2026):
    r = random.Random(seed)
    ont = gen_fastq_ont.generate(40000, seed=8)
    out = []
    for k in range(n):
        size = r.choice((300, 2000, 9000))
        at = r.randrange(0, len(ont) - size)
        data = ont[at:at + size]
        body = bytearray(deflate(data, r.choice((1, 6, 9)), r.choice((zlib.Z_DEFAULT_STRATEGY, zlib.Z_DEFAULT_STRATEGY, zlib.Z_FIXED))))
        bit = r.randrange(0, len(body) * 8)
        body[bit >> 3] ^= 1 << (bit & 7)
        out.append(Case("fuzz%d" % k, frame(body, data), data, "fuzz"))
    return out


def corpus(host_encoder=None, tmpdir=None):
    return valid_cases(host_encoder, tmpdir) + damaged_cases() + fuzz_cases()


def small_members(n, seed=3):
    """n small valid members (for the member-count cases): (member, data) pairs"""
    r = random.Random(seed)
    ont = gen_fastq_ont.generate(30000, seed=9)
    out = []
    for k in range(n):
        size = r.randrange(1, 400)
        at = r.randrange(0, len(ont) - size)
        d = ont[at:at + size]
        out.append((frame(deflate(d, 1 + k % 9), d), d))
    return out


def every_alignment():
    """32 members: a deflated one and a stored one in turn, each pair 1 mod 16 bytes long, so that in a concatenation the deflated
    members start at every alignment mod 16"""
    ont = gen_fastq_ont.generate(30000, seed=10)
    out = []
    for k in range(16):
        d = ont[1000 * k:1000 * k + 700 + 37 * k]
        m = frame(deflate(d), d)
        pad = (1 - len(m) - 31) % 16
        filler = bytes([k]) * pad
        bw = Bits()
        stored_block(bw, filler)
        s = frame(bw.bytes(), filler)
        assert (len(m) + len(s)) % 16 == 1
        out += [(m, d), (s, filler)]
    return out


# ---- the corpus file of tests/bgzf_inflate_host.cpp ---------------------------------------------------------------------------------
def isize_of(member):
    return struct.unpack("<I", member[-4:])[0]


def write_corpus(path, members):
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(members)))
        for m in members:
            f.write(struct.pack("<II", len(m), isize_of(m)))
            f.write(m)


def read_results(path):
    """-> [(status, bytes)]"""
    s, pos, out = open(path, "rb").read(), 0, []
    while pos < len(s):
        st, n = struct.unpack_from("<II", s, pos)
        out.append((st, s[pos + 8:pos + 8 + n]))
        pos += 8 + n
    return out


def check_results(cases, results):
    """the assertions on (status, bytes) per case, shared by the host and the GPU test"""
    assert len(cases) == len(results)
    for c, (st, got) in zip(cases, results):
        if c.kind == "valid":
            assert st == 0, (c.name, st)
            assert got == c.data, c.name
        elif c.kind == "damaged":
            assert st != 0, c.name
        elif st == 0:
            assert zlib_ok(c.member, got), c.name
