"""Unaligned BAM for the tests, written from the SAM/BAM specification (section 4.2) and not from csrc/bam_record.h: a writer, the
FASTQ text a file is expected to give, and a model of the record walk (where it ends and why).

A record is a dict: name (bytes), seq (str over BASES), qual (bytes of Phred values, or None: 0xFF at every position), and
optionally flag, cigar (a tuple of packed operations), tags (bytes)."""
import struct
import zlib

BASES = "=ACMGRSVTWYHKDBN"
COMPLEMENT = dict(zip("=ACMGRSVTWYHKDBN", "=TGKCYSBAWRDMHVN"))
END, TRUNCATED, MALFORMED, HEADER, MORE = range(5)  # FLX_BAM_*


def rec(name, seq, qual, flag=4, cigar=(), tags=b""):
    return {"name": bytes(name), "seq": seq, "qual": None if qual is None else bytes(qual), "flag": flag, "cigar": tuple(cigar), "tags": bytes(tags)}


def pack_bases(seq):
    out = bytearray((len(seq) + 1) // 2)
    for i, ch in enumerate(seq):
        out[i // 2] |= BASES.index(ch) << (0 if i % 2 else 4)
    return bytes(out)


def record_bytes(r, **override):
    """One record as in the file.  override: raw values of block_size / l_read_name / n_cigar_op / l_seq (damaged records)."""
    l = len(r["seq"])
    qual = r["qual"] if r["qual"] is not None else b"\xff" * l
    assert len(qual) == l and len(r["name"]) <= 254
    fixed = struct.pack("<iiBBHHHiiii", -1, -1, override.get("l_read_name", len(r["name"]) + 1), 0, 4680, override.get("n_cigar_op", len(r["cigar"])),
                        r["flag"], override.get("l_seq", l), -1, -1, 0)
    body = fixed + r["name"] + b"\0" + b"".join(struct.pack("<I", c) for c in r["cigar"]) + pack_bases(r["seq"]) + qual + r["tags"]
    return struct.pack("<I", override.get("block_size", len(body))) + body


def header_bytes(text=b"@HD\tVN:1.6\tSO:unsorted\n", refs=()):
    out = b"BAM\1" + struct.pack("<i", len(text)) + text + struct.pack("<i", len(refs))
    for name, length in refs:
        out += struct.pack("<i", len(name) + 1) + name + b"\0" + struct.pack("<i", length)
    return out


def bam_bytes(records, **header):
    """The inflated file."""
    return header_bytes(**header) + b"".join(record_bytes(r) for r in records)


def record_offsets(records, **header):
    off = [len(header_bytes(**header))]
    for r in records:
        off.append(off[-1] + len(record_bytes(r)))
    return off


def bgzf_member(data, level=6):
    assert len(data) <= 65536
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    body = c.compress(data) + c.flush()
    bsize = 18 + len(body) + 8
    assert bsize <= 65536
    return (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", bsize - 1) + body +
            struct.pack("<II", zlib.crc32(data) & 0xffffffff, len(data)))


EOF_BLOCK = bgzf_member(b"")


def bgzf(data, cuts=None, member=65280, level=6, eof=True):
    """BGZF of `data`: members of at most `member` bytes, or one member per piece between the offsets in `cuts`."""
    if cuts is None:
        cuts = list(range(0, len(data), member)) + [len(data)]
    cuts = sorted(set([0, len(data)] + list(cuts)))
    out = b"".join(bgzf_member(data[a:b], level) for a, b in zip(cuts, cuts[1:]))
    return out + (EOF_BLOCK if eof else b"")


def has_text(r):
    return not (r["flag"] & 0x900) and len(r["seq"]) > 0


def expected_record(r):
    seq, qual = r["seq"], r["qual"]
    if qual is None or qual[0] == 0xff:
        q = '"' * len(seq)
    else:
        q = "".join(chr(min(v, 93) + 33) for v in qual)
    if r["flag"] & 0x10:
        seq = "".join(COMPLEMENT[ch] for ch in reversed(seq))
        q = q[::-1]
    return b"@" + r["name"] + b"\n" + seq.encode() + b"\n+\n" + q.encode("latin-1") + b"\n"


def expected_fastq(records):
    """(the text, the text offsets of the records (len + 1), the number of skipped records)"""
    text, off, skipped = bytearray(), [0], 0
    for r in records:
        if has_text(r):
            text += expected_record(r)
        else:
            skipped += 1
        off.append(len(text))
    return bytes(text), off, skipped


def decode_record(data, at):
    """The record dict of a VALID record at data[at:] (for the model below)."""
    bs, = struct.unpack_from("<I", data, at)
    l_name, = struct.unpack_from("<B", data, at + 12)
    n_cigar, flag, l_seq = struct.unpack_from("<HHi", data, at + 16)
    p = at + 36
    name = data[p:p + l_name - 1]
    p += l_name + 4 * n_cigar
    packed = data[p:p + (l_seq + 1) // 2]
    seq = "".join(BASES[(packed[i // 2] >> (0 if i % 2 else 4)) & 15] for i in range(l_seq))
    p += (l_seq + 1) // 2
    return rec(name, seq, data[p:p + l_seq] if l_seq else b"", flag)


def walk_model(data):
    """(records, end state) of an inflated file, by the rules of the specification.  A rule that the bytes present already break
    makes the file MALFORMED (HEADER inside the header); a file that ends before a rule can be checked is TRUNCATED.  Which of
    the two wins where both apply is no matter of the specification but the convention include/filtlong_hip.h documents for
    flx_bam_index, restated here: the tests pin it.  The text, the offsets and the complement table are independent."""
    n = len(data)

    def i32(at):
        return struct.unpack_from("<i", data, at)[0] if at + 4 <= n else None

    for i in range(4):
        if i >= n:
            return [], TRUNCATED
        if data[i] != b"BAM\1"[i]:
            return [], HEADER
    at = 4
    l_text = i32(at)
    if l_text is None:
        return [], TRUNCATED
    if l_text < 0:
        return [], HEADER
    at += 4
    if n - at < l_text:
        return [], TRUNCATED
    at += l_text
    n_ref = i32(at)
    if n_ref is None:
        return [], TRUNCATED
    if n_ref < 0:
        return [], HEADER
    at += 4
    for _ in range(n_ref):
        l_name = i32(at)
        if l_name is None:
            return [], TRUNCATED
        if l_name < 0:
            return [], HEADER
        at += 4
        if n - at < l_name:
            return [], TRUNCATED
        at += l_name
        if n - at < 4:
            return [], TRUNCATED
        at += 4
    records = []
    while True:
        if at >= n:
            return records, END
        if n - at < 4:
            return records, TRUNCATED
        bs, = struct.unpack_from("<I", data, at)
        if bs < 32:
            return records, MALFORMED
        if n - at - 4 < 32:
            return records, TRUNCATED
        l_name = data[at + 12]
        n_cigar, _, l_seq = struct.unpack_from("<HHi", data, at + 16)
        if l_name < 1 or l_seq < 0:
            return records, MALFORMED
        if 32 + l_name + 4 * n_cigar + (l_seq + 1) // 2 + l_seq > bs:
            return records, MALFORMED
        if n - at - 4 < bs:
            return records, TRUNCATED
        if data[at + 36 + l_name - 1] != 0:
            return records, MALFORMED
        records.append(decode_record(data, at))
        at += 4 + bs


def read_fastq(path):
    """The records of a four-line FASTQ file (the reference fixtures) as record dicts; the whole header line is the name.  A BAM
    record has one length: a quality line shorter than the sequence is filled up with its last value."""
    lines = open(path, "rb").read().split(b"\n")
    out = []
    for i in range(0, len(lines) - 3, 4):
        assert lines[i][:1] == b"@" and lines[i + 2][:1] == b"+"
        seq, q = lines[i + 1].decode(), lines[i + 3]
        q = (q + q[-1:] * len(seq))[:len(seq)]
        out.append(rec(lines[i][1:], seq, bytes(c - 33 for c in q)))
    return out
