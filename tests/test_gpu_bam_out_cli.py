"""--bam through the whole command line.  stdout is BGZF whose bytes walk to the end as an unaligned BAM file (tests/_bam.py's model
of the specification); its reads are the reads of the run without --bam, in that order, names without comments; stderr, the exit
status and the --report bytes are that run's.  FASTA input gives 0xFF qualities; --trim --split children are named and cut as in
the text; a BAM input without --trim / --split comes out record for record, byte for byte, tags and header included, and the output
fed back in gives the same reads; --gpus 2 gives the bytes of one GPU; a 255-byte name ends the run before anything is written."""
import gzip
import os
import struct
import subprocess

import pytest

import _bam
import _bam_encode_cases as enc_cases
import _bgzf
import _cases
import _e2e_checks

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "filtlong_amd", "bin", "filtlong")
TEXT_HEADER = _bam.header_bytes(text=b"@HD\tVN:1.6\tSO:unknown\n")
TAGS = b"MMZC+m,5,12,0;\0MLBC" + struct.pack("<I", 3) + b"\x80\x10\xf0" + b"RGZg1\0qsi\x0c\0\0\0"


def run(args, extra=None):
    env = dict(os.environ, LANG="C", LC_ALL="C")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    env.update(extra or {})
    p = subprocess.run([BIN] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
    return p.returncode, p.stdout, p.stderr


def shim_env():
    shim_dir = os.path.join(ROOT, "tests", "shim")
    subprocess.check_call(["make", "-s", "-C", shim_dir])
    return {"FLX_RCCL_LIB": os.path.join(shim_dir, "libloopback_rccl.so"), "FLX_DEVICE": "0"}


def text_without_comments(plain, fasta=False):
    """the plain run's stdout as the text a BAM file of it gives back: names only, bases through the table"""
    lines = plain.split(b"\n")
    step = 2 if fasta else 4
    out = bytearray()
    for i in range(0, len(lines) - 1, step):
        assert lines[i][:1] == (b">" if fasta else b"@")
        seq = "".join(enc_cases.base_of(c) for c in lines[i + 1]).encode()
        qual = b'"' * len(seq) if fasta else lines[i + 3]
        out += b"@" + enc_cases.name_of_header(lines[i][1:]) + b"\n" + seq + b"\n+\n" + qual + b"\n"
    return bytes(out)


def raw_records(data, at):
    out = []
    while at < len(data):
        size = 4 + struct.unpack_from("<I", data, at)[0]
        out.append(data[at:at + size])
        at += size
    assert at == len(data)
    return out


def bam_of(stdout, header=TEXT_HEADER):
    """the decompressed output: a whole BGZF stream with its end-of-file block, the header, records that walk to END"""
    data, info = _bgzf.validate(stdout)
    assert info["eof"] and gzip.decompress(stdout) == data
    assert data[:len(header)] == header
    records, end = _bam.walk_model(data)
    assert end == _bam.END
    return data, records


def same_reads(args, path, extra=None, fasta=False, header=TEXT_HEADER):
    """the run with and without --bam: the same status and stderr, the same reads in the same order -> (plain stdout, BAM bytes)"""
    plain = run(args + [path], extra)
    rc, out, err = run(["--bam"] + args + [path], extra)
    assert plain[0] == 0 and plain[1]
    assert (rc, err) == (plain[0], plain[2]), err[-500:]
    data, records = bam_of(out, header)
    assert _bam.expected_fastq(records)[0] == text_without_comments(plain[1], fasta)
    assert all(r["flag"] == 4 for r in records) or header != TEXT_HEADER
    return plain[1], data


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    d = tmp_path_factory.mktemp("bam_out_inputs")
    f = {}

    def put(name, data):
        (d / name).write_bytes(data)
        f[name] = str(d / name)

    inp = _e2e_checks.Inputs()
    put("phred.fastq", _cases.long_fastq_bytes(inp.preads))  # ("@name extra comment")
    put("phred.fastq.gz", gzip.compress(_cases.long_fastq_bytes(inp.preads)))
    put("kmer.fastq", _cases.long_fastq_bytes(inp.kreads))
    put("ref.fasta", _cases.fasta_bytes(inp.contigs))
    # a BAM input as a basecaller writes it: modified-base tags, one stored reversed, a supplementary record, a header with text
    lines = _cases.c1_fastq_bytes(n=120, length=1500).split(b"\n")
    recs = [_bam.rec(lines[i][1:], lines[i + 1].decode(), bytes(c - 33 for c in lines[i + 3]), tags=TAGS if (i // 4) % 3 else b"")
            for i in range(0, len(lines) - 3, 4)]
    recs[3]["flag"] = 0x10
    recs[5]["flag"] = 0x10 | 0x400
    recs[9]["flag"] = 0x800
    recs[9]["name"] = b"supplementary"
    recs.insert(20, _bam.rec(b"empty", "", b"", tags=TAGS))
    header = dict(text=b"@HD\tVN:1.6\tSO:unsorted\n@RG\tID:g1\tPL:ONT\n@PG\tID:basecaller\n")
    put("tags.bam", _bam.bgzf(_bam.bam_bytes(recs, **header)))
    put("kmer.bam", _bam.bgzf(_bam.bam_bytes([_bam.rec(name.encode(), "".join(enc_cases.base_of(c) for c in s), bytes(c - 33 for c in q), tags=TAGS)
                                              for name, s, q in inp.kreads], **header)))
    f["tags.records"] = recs
    f["tags.header"] = _bam.header_bytes(**header)
    return f


def test_fastq_in(inputs):
    for args in (["--keep_percent", "80"], ["--min_length", "1"]):
        same_reads(args, inputs["phred.fastq"])
    for name in ("test_sort.fastq", "test_split.fastq"):
        same_reads(["--target_bases", "10000"], os.path.join(_cases.FIXTURES, name))


def test_fastq_in_streamed_and_fed_back(inputs, tmp_path):
    plain, data = same_reads(["--keep_percent", "80"], inputs["phred.fastq"])
    assert same_reads(["--keep_percent", "80"], inputs["phred.fastq.gz"])[1] == data  # (a gzip input is streamed: the other output pass)
    # closure: the output as an input gives the reads the original gives, names without their comments
    back = tmp_path / "back.bam"
    back.write_bytes(run(["--bam", "--min_length", "1", inputs["phred.fastq"]])[1])
    rc, out, err = run(["--keep_percent", "80", str(back)])
    assert rc == 0 and out == text_without_comments(plain)


def test_fasta_in(inputs):
    fasta = os.path.join(_cases.FIXTURES, "test_sort.fasta")
    plain, data = same_reads(["-a", os.path.join(_cases.FIXTURES, "test_reference.fasta"), "--min_length", "1"], fasta, fasta=True)
    recs = raw_records(data, len(TEXT_HEADER))
    assert recs
    for raw in recs:
        l_seq, = struct.unpack_from("<i", raw, 20)
        assert l_seq > 0 and raw[-l_seq:] == b"\xff" * l_seq  # no qualities stored, no tags behind them


def test_trim_split_children(inputs):
    plain, data = same_reads(["-a", inputs["ref.fasta"], "--trim", "--split", "100", "--keep_percent", "80"], inputs["kmer.fastq"])
    names = [l[1:].split(b" ")[0] for l in plain.split(b"\n")[0::4] if l]
    assert any(b"_" in n and b"-" in n.rsplit(b"_", 1)[-1] for n in names)  # children, named with their coordinates


def test_bam_in_with_tags(inputs, tmp_path):
    by_name = {r["name"]: _bam.record_bytes(r) for r in inputs["tags.records"]}
    for args in (["--keep_percent", "70"], ["--min_length", "1"]):
        plain = run(args + [inputs["tags.bam"]])
        rc, out, err = run(["--bam"] + args + [inputs["tags.bam"]])
        assert plain[0] == 0 and (rc, err) == (0, plain[2])
        data, records = bam_of(out, inputs["tags.header"])
        kept = [l[1:] for l in plain[1].split(b"\n")[0::4] if l]
        # the original records of the reads the plain run keeps, in its order: block_size through the last tag
        assert raw_records(data, len(inputs["tags.header"])) == [by_name[n] for n in kept]
        assert b"supplementary" not in kept and b"empty" not in kept and len(kept) > 50
        if args[0] == "--min_length":
            assert kept[3] == inputs["tags.records"][3]["name"] and any(TAGS in by_name[n] for n in kept)
    # closure: the output as an input gives the plain stdout of the original input
    back = tmp_path / "back.bam"
    back.write_bytes(run(["--bam", "--min_length", "1", inputs["tags.bam"]])[1])
    want = run(["--keep_percent", "70", inputs["tags.bam"]])
    got = run(["--keep_percent", "70", str(back)])
    assert got[0] == 0 and got[1] == want[1] and want[1]


def test_bam_in_with_trim_and_split_is_encoded_from_text(inputs):
    args = ["-a", inputs["ref.fasta"], "--trim", "--split", "100", "--keep_percent", "80"]
    plain = run(args + [inputs["kmer.bam"]])
    rc, out, err = run(["--bam"] + args + [inputs["kmer.bam"]])
    assert plain[0] == 0 and plain[1] and (rc, err) == (0, plain[2])
    data, records = bam_of(out, inputs["tags.header"])
    # whole reads and children alike: named and cut as the text names and cuts them, unmapped, and no tag survives
    assert _bam.expected_fastq(records)[0] == text_without_comments(plain[1])
    assert all(r["flag"] == 4 for r in records) and b"MMZ" not in data
    assert any(b"_" in r["name"] and b"-" in r["name"].rsplit(b"_", 1)[-1] for r in records)


def test_two_ranks(inputs):
    extra = shim_env()
    for args, path in ((["--target_bases", "300000"], inputs["phred.fastq"]), (["--keep_percent", "70"], inputs["tags.bam"])):
        one = run(["--bam"] + args + [path])
        two = run(["--bam", "--gpus", "2"] + args + [path], extra)
        assert one[0] == two[0] == 0
        assert _bgzf.validate(two[1])[0] == _bgzf.validate(one[1])[0] and len(one[1]) > 28
        assert two[2] == run(["--gpus", "2"] + args + [path], extra)[2]


def test_report(inputs, tmp_path):
    got = {}
    for flag in ((), ("--bam",)):
        rep = tmp_path / ("report%d.json" % len(flag))
        rc, out, err = run(list(flag) + ["--report", str(rep), "--keep_percent", "70", inputs["phred.fastq"]])
        assert rc == 0
        got[flag] = (rep.read_bytes(), err)
    assert got[()] == got[("--bam",)] and got[()][0]


def test_a_name_bam_cannot_hold(inputs, tmp_path):
    seq = b"ACGT" * 500
    reads = [(b"ok_%d" % i, seq) for i in range(40)]
    reads[31] = (b"n" * 255, seq)
    path = tmp_path / "long_name.fastq"
    path.write_bytes(b"".join(b"@" + n + b"\n" + s + b"\n+\n" + b"I" * len(s) + b"\n" for n, s in reads))
    for extra_args, extra in (([], None), (["--gpus", "2"], shim_env())):
        assert run(extra_args + ["--min_length", "1", str(path)], extra)[0] == 0  # (text takes any name)
        rc, out, err = run(["--bam"] + extra_args + ["--min_length", "1", str(path)], extra)
        assert rc == 1 and out == b"" and err.endswith(b"Error: read name cannot be written as BAM: " + b"n" * 255 + b"\n"), (extra_args, err[-400:])
    reads[31] = (b"m" * 254, seq)
    path.write_bytes(b"".join(b"@" + n + b"\n" + s + b"\n+\n" + b"I" * len(s) + b"\n" for n, s in reads))
    same_reads(["--min_length", "1"], str(path))
