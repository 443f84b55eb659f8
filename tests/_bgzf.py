"""A strict pure-Python BGZF validator (SAM/BAM specification §4.1) and a BGZF writer built on zlib, for the tests.

validate(stream) walks the members: the fixed gzip header bytes, XLEN 6 with the single `BC` subfield of length 2, BSIZE
equal to the member's size - 1, the deflate data inflated by zlib.decompressobj(-15) ending exactly at the trailer,
CRC-32 and ISIZE of what it inflated.  It returns the concatenated contents and facts about the members, and raises
BgzfError at the first thing that is not right.
"""
import struct
import zlib

MEMBER = 65280  # input bytes per member (bgzip's BGZF_BLOCK_SIZE)
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
HEADER = bytes.fromhex("1f8b08040000000000ff06004243") + b"\x02\x00"  # up to BSIZE


class BgzfError(ValueError):
    pass


def validate(stream, require_eof=True, max_member=65536):
    """-> (data, info) with info = {"members": [(offset, size, isize), ...], "eof": bool}"""
    stream = bytes(stream)
    pos, out, members, eof = 0, [], [], False
    while pos < len(stream):
        if len(stream) - pos < 26:
            raise BgzfError("truncated member at %d" % pos)
        if stream[pos:pos + 16] != HEADER:
            raise BgzfError("bad member header at %d: %s" % (pos, stream[pos:pos + 16].hex()))
        bsize = struct.unpack_from("<H", stream, pos + 16)[0] + 1
        if bsize < 26 or bsize > max_member or pos + bsize > len(stream):
            raise BgzfError("bad BSIZE %d at %d" % (bsize, pos))
        member = stream[pos:pos + bsize]
        d = zlib.decompressobj(-15)
        try:
            data = d.decompress(member[18:])
        except zlib.error as e:
            raise BgzfError("deflate data of the member at %d: %s" % (pos, e))
        if not d.eof:
            raise BgzfError("deflate data of the member at %d does not end" % pos)
        if len(d.unused_data) != 8:
            raise BgzfError("deflate data of the member at %d ends %d bytes before its end (want 8)" % (pos, len(d.unused_data)))
        crc, isize = struct.unpack("<II", d.unused_data)
        if crc != zlib.crc32(data):
            raise BgzfError("CRC-32 of the member at %d" % pos)
        if isize != len(data):
            raise BgzfError("ISIZE of the member at %d" % pos)
        if isize == 0:
            if member != EOF_BLOCK or pos + bsize != len(stream):
                raise BgzfError("empty member at %d is not the final end-of-file block" % pos)
            eof = True
        members.append((pos, bsize, isize))
        out.append(data)
        pos += bsize
    if require_eof and not eof:
        raise BgzfError("no end-of-file block")
    return b"".join(out), {"members": members, "eof": eof}


def zlib_bgzf(data, level, eof=True):
    """BGZF of `data` on the same 65280-byte grid, each member deflated by zlib at `level` (the size yardstick)."""
    out = []
    for k in range(0, len(data), MEMBER):
        chunk = data[k:k + MEMBER]
        c = zlib.compressobj(level, zlib.DEFLATED, -15)
        body = c.compress(chunk) + c.flush()
        size = 18 + len(body) + 8
        out.append(HEADER + struct.pack("<H", size - 1) + body + struct.pack("<II", zlib.crc32(chunk), len(chunk)))
    if eof:
        out.append(EOF_BLOCK)
    return b"".join(out)
