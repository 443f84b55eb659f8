"""--bam on the command line, without a GPU: the flag is one of this binary's own like --gzip, the two together are refused with
their message and status 1 behind the reference's own checks, and --bam alone passes the argument parser — under
FLX_CLI_PARSE_ONLY the run gives the digest it gives without the flag, and without that switch a machine with no device fails for
the device, never with "flag could not be matched"."""
import os
import subprocess

import pytest

import _cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "filtlong_amd", "bin", "filtlong")
FASTQ = os.path.join(_cases.FIXTURES, "test_sort.fastq")


@pytest.fixture(scope="module")
def binary():
    if not os.path.exists(BIN):
        import __graft_entry__
        __graft_entry__.build()
    return BIN


def run(args, extra=None):
    env = dict(os.environ, LANG="C", LC_ALL="C")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "FLX_CLI_PARSE_ONLY"):
        env.pop(k, None)
    env.update(extra or {})
    p = subprocess.run([BIN] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
    return p.returncode, p.stdout, p.stderr


def test_gzip_and_bam_are_refused_together(binary):
    for args in (["--gzip", "--bam"], ["--bam", "--gzip"]):
        rc, out, err = run(args + ["--min_length", "1", FASTQ])
        assert (rc, out, err) == (1, b"", b"Error: --gzip and --bam cannot be used together\n")


def test_the_refusal_comes_behind_the_checks_of_the_reference(binary):
    # every one of these fails as it does without the two flags: the new check does not change their order
    for args in (["--min_length", "1", "/no/such/file.fastq"], [FASTQ], ["--min_length", "0", FASTQ], ["--trim", "--min_length", "1", FASTQ],
                 ["--window_size", "0", "--min_length", "1", FASTQ], ["--gpus", "0", "--min_length", "1", FASTQ]):
        want = run(args)
        assert want[0] == 1 and want[2]
        assert run(["--gzip", "--bam"] + args) == want, args


def test_bam_alone_passes_the_parser(binary):
    want = run(["--min_length", "1", FASTQ], {"FLX_CLI_PARSE_ONLY": "seq"})
    got = run(["--bam", "--min_length", "1", FASTQ], {"FLX_CLI_PARSE_ONLY": "seq"})
    assert want[0] == 0 and got == want
    # the whole run: with a device it succeeds, without one it fails for the device — never in the argument parser
    rc, out, err = run(["--bam", "--min_length", "1", FASTQ])
    assert b"flag could not be matched" not in err and b"cannot be used together" not in err
    assert rc == 0 or (rc == 1 and out == b"")


def test_help_stays_the_menu_of_the_reference(binary):
    rc, out, err = run(["--help"])
    assert rc == 0 and b"--bam" not in out + err and b"--gzip" not in out + err
