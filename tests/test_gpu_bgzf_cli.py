"""`filtlong --gzip` on the GPU: stdout is a BGZF stream (strictly valid, ending in the end-of-file block) whose contents are
byte for byte the stdout of the same command without --gzip; stderr and the exit status are those of the plain run.  The plain
run is the yardstick here; the other CLI tests tie it to the reference."""
import gzip
import os
import subprocess

import pytest

import _bgzf
import _cases
import _e2e_checks

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "filtlong_amd", "bin", "filtlong")
FIX = _cases.FIXTURES
BLOCKS = {"FLX_CLI_FORCE_STREAM": "1", "FLX_CLI_BLOCK_BYTES": "6000", "FLX_CLI_PINFLATE_MIN": "1", "FLX_CLI_PINFLATE_CHUNK": "2000"}


def env_of(extra=None):
    env = dict(os.environ, LANG="C", LC_ALL="C")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    env.update(extra or {})
    return env


def run(args, tmp_path, extra=None, to_file=False, tag="out"):
    if to_file:
        path = tmp_path / (tag + ".bin")
        with open(path, "wb") as fh:
            p = subprocess.run([BIN] + args, stdout=fh, stderr=subprocess.PIPE, env=env_of(extra))
        return p.returncode, path.read_bytes(), p.stderr
    p = subprocess.run([BIN] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env_of(extra))
    return p.returncode, p.stdout, p.stderr


def same_as_plain(args, tmp_path, extra=None, to_file=False, prefix=()):
    rc, plain, err = run(list(prefix) + args, tmp_path, extra, to_file, "plain")
    rcz, z, errz = run(list(prefix) + ["--gzip"] + args, tmp_path, extra, to_file, "gz")
    assert (rcz, errz) == (rc, err), (args, errz[-400:], err[-400:])
    if rc == 0:
        got, info = _bgzf.validate(z)
        assert z.endswith(_bgzf.EOF_BLOCK)
    else:  # an error after some output: what was written is still whole members
        got, info = _bgzf.validate(z, require_eof=False)
    assert got == plain, args
    assert gzip.decompress(z) == plain if z else plain == b""
    return rc, plain, z


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    d = tmp_path_factory.mktemp("inputs")
    fq = d / "c1.fastq"
    fq.write_bytes(_cases.c1_fastq_bytes(n=3000))
    inp = _e2e_checks.Inputs()
    kfq = d / "kmer.fastq"
    kfq.write_bytes(_cases.long_fastq_bytes(inp.kreads))
    fa = d / "ref.fasta"
    fa.write_bytes(_cases.fasta_bytes(inp.contigs))
    gz = d / "c1.fastq.gz"
    gz.write_bytes(gzip.compress(fq.read_bytes(), 1))
    return {"fq": str(fq), "kfq": str(kfq), "fa": str(fa), "gz": str(gz), "dir": d}


def test_phred_modes(tmp_path, inputs):
    rc, plain, _ = same_as_plain(["--target_bases", "5000000", inputs["fq"]], tmp_path)
    assert rc == 0 and len(plain) > 1_000_000
    same_as_plain(["--target_bases", "5000000", inputs["fq"]], tmp_path, to_file=True)
    same_as_plain(["--min_length", "1000", "--keep_percent", "90", os.path.join(FIX, "test_sort.fastq")], tmp_path)
    same_as_plain(["--verbose", "--min_mean_q", "10", os.path.join(FIX, "test_trim.fastq")], tmp_path)


def test_kmer_modes(tmp_path, inputs):
    rc, plain, _ = same_as_plain(["-a", inputs["fa"], "--trim", "--split", "100", "--keep_percent", "80", inputs["kfq"]], tmp_path)
    assert rc == 0 and plain
    same_as_plain(["-1", os.path.join(FIX, "test_reference_1.fastq.gz"), "-2", os.path.join(FIX, "test_reference_2.fastq.gz"),
                   "--trim", "--split", "50", "--min_length", "100", os.path.join(FIX, "test_split.fastq")], tmp_path)
    # FASTA in, FASTA out
    fasta = inputs["dir"] / "reads.fasta"
    fasta.write_bytes(_cases.fasta_bytes(_e2e_checks.Inputs().contigs, prefix="r"))
    same_as_plain(["-a", inputs["fa"], "--min_length", "10", str(fasta)], tmp_path)


def test_streamed_gzip_input(tmp_path, inputs):
    rc, plain, _ = same_as_plain(["--target_bases", "5000000", inputs["gz"]], tmp_path, BLOCKS)
    assert rc == 0 and plain
    same_as_plain(["--target_bases", "5000000", inputs["gz"]], tmp_path)


def test_damaged_gzip_input(tmp_path, inputs):
    blob = open(inputs["gz"], "rb").read()
    for cut in (len(blob) // 3, len(blob) - 9):
        bad = tmp_path / ("cut%d.fastq.gz" % cut)
        bad.write_bytes(blob[:cut])
        for extra in (None, BLOCKS):
            same_as_plain(["--min_length", "1", str(bad)], tmp_path, extra)


def test_no_read_passes(tmp_path, inputs):
    rc, plain, z = same_as_plain(["--min_length", "100000000", inputs["fq"]], tmp_path)
    assert rc == 0 and plain == b"" and z == _bgzf.EOF_BLOCK


@pytest.mark.parametrize("gpus", ["2", "3"])
def test_forked_ranks(tmp_path, inputs, gpus):
    shim_dir = os.path.join(ROOT, "tests", "shim")
    subprocess.check_call(["make", "-s", "-C", shim_dir])
    extra = {"FLX_RCCL_LIB": os.path.join(shim_dir, "libloopback_rccl.so"), "FLX_DEVICE": "0"}
    for to_file in (False, True):
        rc, plain, z = same_as_plain(["--target_bases", "5000000", inputs["fq"]], tmp_path, extra, to_file, ["--gpus", gpus])
        assert rc == 0 and plain
        assert z.count(_bgzf.EOF_BLOCK) == 1 and z.endswith(_bgzf.EOF_BLOCK)
    same_as_plain(["-a", inputs["fa"], "--trim", "--split", "100", "--keep_percent", "80", inputs["kfq"]], tmp_path, extra, True,
                  ["--gpus", gpus])


def test_output_read_back_by_the_cli(tmp_path, inputs):
    rc, z, _ = run(["--gzip", "--min_length", "1", inputs["fq"]], tmp_path)
    assert rc == 0
    back = tmp_path / "back.fastq.gz"
    back.write_bytes(z)
    plain_rc, plain, plain_err = run(["--min_length", "1", inputs["fq"]], tmp_path)
    assert gzip.decompress(z) == plain
    for extra in (None, BLOCKS):
        rc2, again, _ = run(["--min_length", "1", str(back)], tmp_path, extra)
        assert rc2 == 0 and again == plain
