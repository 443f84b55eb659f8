"""--exclude / --exclude_percent on the command line, as far as it goes without a GPU: arguments are judged before any device is asked
for.  The flags' three argument errors come behind every check of the reference and of --split_window_q (status 1, nothing on stdout),
--exclude alone counts as a threshold, and --help stays the reference's menu.  (The fourth message, too many 16-mers, needs the set:
tests/test_exclude_cli_gpu.py.)"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "filtlong_amd", "bin", "filtlong")
FASTQ = os.path.join(ROOT, "tests", "golden", "ref_fixtures", "test_sort.fastq")
FASTA = os.path.join(ROOT, "tests", "golden", "ref_fixtures", "test_reference.fasta")
NO_THRESHOLDS = b"Error: no thresholds set, you must use one of the following options:\ntarget_bases, keep_percent, min_length, max_length, min_mean_q, min_window_q, trim, split\n"
BAD_PERCENT = b"Error: the value for --exclude_percent must be greater than 0 and at most 100\n"
ENV_ANSWER = b"Error: unknown environment variable FLX_CLI_NO_SUCH_SWITCH (the FLX_CLI_* switches are listed in README.md)\n"


@pytest.fixture(scope="module")
def exe():
    if not os.path.exists(EXE):
        import __graft_entry__
        __graft_entry__.build()
    return EXE


def run(exe, *args, env=None):
    return subprocess.run([exe] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)


def accepted(exe, *args):
    """the arguments pass: the run goes on to the environment check, which answers before any device is asked for"""
    p = run(exe, *args, env=dict(os.environ, FLX_CLI_NO_SUCH_SWITCH="1"))
    return p.returncode == 1 and p.stdout == b"" and p.stderr == ENV_ANSWER


def test_missing_file(exe):
    p = run(exe, "--exclude", FASTA + ".missing", FASTQ)
    assert p.returncode == 1 and p.stdout == b""
    assert p.stderr == b"Error: cannot find file: " + (FASTA + ".missing").encode() + b"\n"


@pytest.mark.parametrize("value", ["0", "0.0", "100.5", "101", "1000"])
def test_percent_out_of_range(exe, value):
    p = run(exe, "--exclude", FASTA, "--exclude_percent", value, FASTQ)
    assert p.returncode == 1 and p.stdout == b"" and p.stderr == BAD_PERCENT


@pytest.mark.parametrize("value", ["100", "100.0", "0.001", "10", "60"])
def test_percent_in_range(exe, value):
    assert accepted(exe, "--exclude", FASTA, "--exclude_percent", value, FASTQ)


def test_percent_needs_exclude(exe):
    p = run(exe, "--exclude_percent", "20", "--min_length", "100", FASTQ)
    assert p.returncode == 1 and p.stdout == b"" and p.stderr == b"Error: --exclude_percent needs --exclude\n"
    # ... and the value is judged first
    p = run(exe, "--exclude_percent", "0", "--min_length", "100", FASTQ)
    assert p.returncode == 1 and p.stderr == BAD_PERCENT
    # ... and the file before the value
    p = run(exe, "--exclude", FASTA + ".missing", "--exclude_percent", "0", FASTQ)
    assert p.returncode == 1 and p.stderr.startswith(b"Error: cannot find file: ")


def test_the_new_checks_come_last(exe):
    bad = ["--exclude", FASTA + ".missing", "--exclude_percent", "0"]
    # every message of the reference wins over the flags' own
    p = run(exe, *bad, "--min_length", "0", FASTQ)
    assert p.returncode == 1 and p.stderr == b"Error: the value for --min_length must be a positive integer\n"
    p = run(exe, *bad, "--window_size", "0", FASTQ)
    assert p.returncode == 1 and p.stderr == b"Error: the value for --window_size must be a positive integer\n"
    p = run(exe, *bad, "--keep_percent", "100", FASTQ)
    assert p.returncode == 1 and p.stderr == b"Error: the value for --keep_percent must be greater than 0 and less than 100\n"
    p = run(exe, *bad, "--gzip", "--bam", FASTQ)
    assert p.returncode == 1 and p.stderr == b"Error: --gzip and --bam cannot be used together\n"
    p = run(exe, *bad, "--trim", FASTQ)
    assert p.returncode == 1 and p.stderr == b"Error: assembly or read reference is required to use --trim\n"
    p = run(exe, *bad, FASTQ + ".missing")
    assert p.returncode == 1 and p.stderr == b"Error: cannot find file: " + (FASTQ + ".missing").encode() + b"\n"
    # ... and so do those of --split_window_q
    p = run(exe, *bad, "--split_window_q", "0", FASTQ)
    assert p.returncode == 1 and p.stderr == b"Error: the value for --split_window_q must be greater than 0 and less than 100\n"
    p = run(exe, *bad, "--split_window_q", "85", "-a", FASTA, FASTQ)
    assert p.returncode == 1 and p.stderr == b"Error: --split_window_q cannot be used with an external reference\n"
    # the readers' own messages
    p = run(exe, "--exclude", FASTA, "--exclude_percent", "abc", FASTQ)
    assert p.returncode == 1 and p.stderr == b"Error: argument 'float' received invalid value type 'abc'\n"
    p = run(exe, "--exclude", FASTA, "--exclude_percent", "-5", FASTQ)
    assert p.returncode == 1 and p.stderr == b"Error: argument 'float' received invalid value type '-5'\n"
    p = run(exe, FASTQ, "--exclude")
    assert p.returncode == 1 and p.stderr == b"Error: flag 'exclude' requires an argument but received none\n"
    p = run(exe, FASTQ, "--exclude", FASTA, "--exclude_percent")
    assert p.returncode == 1 and p.stderr == b"Error: flag 'exclude_percent' requires an argument but received none\n"


def test_the_flag_alone_is_a_threshold(exe):
    p = run(exe, FASTQ)
    assert p.returncode == 1 and p.stderr == NO_THRESHOLDS
    assert accepted(exe, "--exclude", FASTA, FASTQ)
    # with every mode it is meant to work with: the arguments are accepted
    assert accepted(exe, "--exclude", FASTA, "-a", FASTA, "--trim", "--split", "100", FASTQ)
    assert accepted(exe, "--exclude", FASTA, "--split_window_q", "85", "--gzip", "--verbose", "--gpus", "2", FASTQ)
    assert accepted(exe, "--exclude", FASTA, "--bam", "--keep_percent", "70", FASTQ)


def test_report_file_must_not_be_the_exclude_file(exe, tmp_path):
    fa = tmp_path / "x.fa"
    fa.write_bytes(b">x\nACGTACGTACGTACGTACGT\n")
    p = run(exe, "--exclude", str(fa), "--report", str(fa), FASTQ)
    assert p.returncode == 1 and p.stdout == b"" and p.stderr == b"Error: report file is one of the input files: " + str(fa).encode() + b"\n"
    assert fa.read_bytes() == b">x\nACGTACGTACGTACGTACGT\n"


def test_help_is_the_reference_menu(exe):
    p = run(exe, "--help")
    assert p.returncode == 0 and b"exclude" not in p.stderr and b"--min_window_q [float]" in p.stderr
