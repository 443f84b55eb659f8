"""--max_low_complexity / --low_complexity_score on the command line, as far as it goes without a GPU: arguments are judged before any
device is asked for.  The flags' three argument errors come behind every check of the reference and of the other own flags — those of
--exclude_k and of the adapters included — in a fixed order (status 1, nothing on stdout), --max_low_complexity alone counts as a
threshold, and --help stays the reference's menu."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "filtlong_amd", "bin", "filtlong")
FASTQ = os.path.join(ROOT, "tests", "golden", "ref_fixtures", "test_sort.fastq")
FASTA = os.path.join(ROOT, "tests", "golden", "ref_fixtures", "test_reference.fasta")
NO_THRESHOLDS = b"Error: no thresholds set, you must use one of the following options:\ntarget_bases, keep_percent, min_length, max_length, min_mean_q, min_window_q, trim, split\n"
BAD_PERCENT = b"Error: the value for --max_low_complexity must be greater than 0 and at most 100\n"
BAD_SCORE = b"Error: the value for --low_complexity_score must be an integer between 10 and 300\n"
NEEDS = b"Error: --low_complexity_score needs --max_low_complexity\n"
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


@pytest.mark.parametrize("value", ["0", "0.0", "100.5", "101", "1000"])
def test_percent_out_of_range(exe, value):
    p = run(exe, "--max_low_complexity", value, FASTQ)
    assert p.returncode == 1 and p.stdout == b"" and p.stderr == BAD_PERCENT


@pytest.mark.parametrize("value", ["100", "100.0", "0.001", "50", "7.5"])
def test_percent_in_range(exe, value):
    assert accepted(exe, "--max_low_complexity", value, FASTQ)


@pytest.mark.parametrize("value", ["9", "301", "0", "20.5", "abc", "-20", "1000000", ""])
def test_score_out_of_range(exe, value):
    p = run(exe, "--max_low_complexity", "50", "--low_complexity_score", value, FASTQ)
    assert p.returncode == 1 and p.stdout == b"" and p.stderr == BAD_SCORE


@pytest.mark.parametrize("value", ["10", "20", "37", "300", "020"])
def test_score_in_range(exe, value):
    assert accepted(exe, "--max_low_complexity", "50", "--low_complexity_score", value, FASTQ)


def test_score_needs_the_filter(exe):
    p = run(exe, "--low_complexity_score", "20", "--min_length", "100", FASTQ)
    assert p.returncode == 1 and p.stdout == b"" and p.stderr == NEEDS
    # ... and the value is judged first
    p = run(exe, "--low_complexity_score", "5", "--min_length", "100", FASTQ)
    assert p.returncode == 1 and p.stdout == b"" and p.stderr == BAD_SCORE
    # ... and the percentage before the score
    p = run(exe, "--max_low_complexity", "0", "--low_complexity_score", "5", FASTQ)
    assert p.returncode == 1 and p.stdout == b"" and p.stderr == BAD_PERCENT


def test_the_new_checks_come_last(exe):
    bad = ["--max_low_complexity", "0", "--low_complexity_score", "5"]
    # every message of the reference wins over the flags' own
    p = run(exe, *bad, "--min_length", "0", FASTQ)
    assert p.returncode == 1 and p.stderr == b"Error: the value for --min_length must be a positive integer\n"
    p = run(exe, *bad, "--window_size", "0", FASTQ)
    assert p.returncode == 1 and p.stderr == b"Error: the value for --window_size must be a positive integer\n"
    p = run(exe, *bad, "--gzip", "--bam", FASTQ)
    assert p.returncode == 1 and p.stderr == b"Error: --gzip and --bam cannot be used together\n"
    p = run(exe, *bad, "--trim", FASTQ)
    assert p.returncode == 1 and p.stderr == b"Error: assembly or read reference is required to use --trim\n"
    p = run(exe, *bad, FASTQ + ".missing")
    assert p.returncode == 1 and p.stderr == b"Error: cannot find file: " + (FASTQ + ".missing").encode() + b"\n"
    # ... and so do those of the other own flags, the last of them included
    p = run(exe, *bad, "--split_window_q", "0", FASTQ)
    assert p.returncode == 1 and p.stderr == b"Error: the value for --split_window_q must be greater than 0 and less than 100\n"
    p = run(exe, *bad, "--exclude", FASTA, "--exclude_percent", "0", FASTQ)
    assert p.returncode == 1 and p.stderr == b"Error: the value for --exclude_percent must be greater than 0 and at most 100\n"
    p = run(exe, *bad, "--trim_adapters", FASTA, "--adapter_errors", "41", FASTQ)
    assert p.returncode == 1 and p.stderr == b"Error: the value for --adapter_errors must be an integer between 0 and 40\n"
    p = run(exe, *bad, "--split_adapters", FASTQ)
    assert p.returncode == 1 and p.stderr == b"Error: --split_adapters needs --trim_adapters\n"
    p = run(exe, *bad, "--trim_adapters", FASTA, "--split_adapters", "--adapter_split_errors", "41", FASTQ)
    assert p.returncode == 1 and p.stderr == b"Error: the value for --adapter_split_errors must be an integer between 0 and 40\n"
    p = run(exe, *bad, "--exclude", FASTA, "--exclude_k", "32", FASTQ)
    assert p.returncode == 1 and p.stderr == b"Error: the value for --exclude_k must be an integer between 16 and 31\n"
    p = run(exe, *bad, "--exclude_k", "20", FASTQ)
    assert p.returncode == 1 and p.stderr == b"Error: --exclude_k needs --exclude\n"
    # ... and with those in order the flags' own answer
    p = run(exe, *bad, "--exclude", FASTA, "--exclude_k", "20", FASTQ)
    assert p.returncode == 1 and p.stdout == b"" and p.stderr == BAD_PERCENT
    # the readers' own messages
    p = run(exe, "--max_low_complexity", "abc", FASTQ)
    assert p.returncode == 1 and p.stderr == b"Error: argument 'float' received invalid value type 'abc'\n"
    p = run(exe, "--max_low_complexity", "-5", FASTQ)
    assert p.returncode == 1 and p.stderr == b"Error: argument 'float' received invalid value type '-5'\n"
    p = run(exe, FASTQ, "--max_low_complexity")
    assert p.returncode == 1 and p.stderr == b"Error: flag 'max_low_complexity' requires an argument but received none\n"
    p = run(exe, FASTQ, "--max_low_complexity", "50", "--low_complexity_score")
    assert p.returncode == 1 and p.stderr == b"Error: flag 'low_complexity_score' requires an argument but received none\n"


def test_the_flag_alone_is_a_threshold(exe):
    p = run(exe, FASTQ)
    assert p.returncode == 1 and p.stderr == NO_THRESHOLDS
    p = run(exe, "--low_complexity_score", "20", FASTQ)  # the score alone is none
    assert p.returncode == 1 and p.stderr == NO_THRESHOLDS
    assert accepted(exe, "--max_low_complexity", "50", FASTQ)
    # with every mode it is meant to work with: the arguments are accepted
    assert accepted(exe, "--max_low_complexity", "50", "-a", FASTA, "--trim", "--split", "100", FASTQ)
    assert accepted(exe, "--max_low_complexity", "50", "-1", FASTQ, "-2", FASTQ, FASTQ)
    assert accepted(exe, "--max_low_complexity", "50", "--split_window_q", "85", "--gzip", "--verbose", "--gpus", "2", FASTQ)
    assert accepted(exe, "--max_low_complexity", "50", "--exclude", FASTA, "--exclude_k", "21", "--bam", "--keep_percent", "70", FASTQ)
    assert accepted(exe, "--max_low_complexity", "50", "--trim_adapters", FASTA, "--split_adapters", "--report", os.devnull, FASTQ)


def test_help_is_the_reference_menu(exe):
    p = run(exe, "--help")
    assert p.returncode == 0 and b"complexity" not in p.stderr and b"--min_window_q [float]" in p.stderr
    q = run(exe, "--max_low_complexity", "50", "--help")
    assert q.returncode == 0 and q.stderr == p.stderr and q.stdout == p.stdout
