"""--trim_ends_q on the command line, as far as it goes without a GPU: arguments are judged before any device is asked for.  The flag's
four argument errors come behind every check of the reference and of the other own flags — those of --adapter_overhang included — in a
fixed order (status 1, nothing on stdout), the flag alone counts as a threshold, and --help stays the reference's menu."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "filtlong_amd", "bin", "filtlong")
FASTQ = os.path.join(ROOT, "tests", "golden", "ref_fixtures", "test_sort.fastq")
FASTA = os.path.join(ROOT, "tests", "golden", "ref_fixtures", "test_reference.fasta")
NO_THRESHOLDS = b"Error: no thresholds set, you must use one of the following options:\ntarget_bases, keep_percent, min_length, max_length, min_mean_q, min_window_q, trim, split\n"
BAD_VALUE = b"Error: the value for --trim_ends_q must be greater than 0 and less than 100\n"
WITH_REFERENCE = b"Error: --trim_ends_q cannot be used with an external reference\n"
WITH_QSPLIT = b"Error: --trim_ends_q cannot be used with --split_window_q\n"
WITH_ADAPTERS = b"Error: --trim_ends_q cannot be used with --trim_adapters\n"
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


@pytest.mark.parametrize("value", ["0", "0.0", "100", "100.0", "101", "1000"])
def test_value_out_of_range(exe, value):
    p = run(exe, "--trim_ends_q", value, FASTQ)
    assert p.returncode == 1 and p.stdout == b"" and p.stderr == BAD_VALUE


@pytest.mark.parametrize("value", ["0.001", "50", "90", "99.9", "7.5"])
def test_value_in_range(exe, value):
    assert accepted(exe, "--trim_ends_q", value, FASTQ)


def test_the_four_messages_in_their_order(exe):
    # the value first, whatever else is wrong
    for rest in (["-a", FASTA], ["--split_window_q", "50"], ["--trim_adapters", FASTA]):
        p = run(exe, "--trim_ends_q", "0", *rest, FASTQ)
        assert p.returncode == 1 and p.stdout == b"" and p.stderr == BAD_VALUE
    # then the external reference: an assembly, or short reads
    p = run(exe, "--trim_ends_q", "90", "-a", FASTA, FASTQ)
    assert p.returncode == 1 and p.stdout == b"" and p.stderr == WITH_REFERENCE
    p = run(exe, "--trim_ends_q", "90", "-1", FASTQ, "-2", FASTQ, FASTQ)
    assert p.returncode == 1 and p.stdout == b"" and p.stderr == WITH_REFERENCE
    # then --split_window_q, in front of --trim_adapters
    p = run(exe, "--trim_ends_q", "90", "--split_window_q", "50", FASTQ)
    assert p.returncode == 1 and p.stdout == b"" and p.stderr == WITH_QSPLIT
    p = run(exe, "--trim_ends_q", "90", "--trim_adapters", FASTA, FASTQ)
    assert p.returncode == 1 and p.stdout == b"" and p.stderr == WITH_ADAPTERS
    p = run(exe, "--trim_adapters", FASTA, "--split_adapters", "--adapter_overhang", "10", "--trim_ends_q", "90", FASTQ)
    assert p.returncode == 1 and p.stdout == b"" and p.stderr == WITH_ADAPTERS


def test_the_new_checks_come_last(exe):
    bad = ["--trim_ends_q", "0"]
    # every message of the reference wins over the flag's own
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
    p = run(exe, *bad, "-a", FASTA, "--split_window_q", "50", FASTQ)
    assert p.returncode == 1 and p.stderr == b"Error: --split_window_q cannot be used with an external reference\n"
    p = run(exe, *bad, "--exclude", FASTA, "--exclude_percent", "0", FASTQ)
    assert p.returncode == 1 and p.stderr == b"Error: the value for --exclude_percent must be greater than 0 and at most 100\n"
    p = run(exe, *bad, "--trim_adapters", FASTA, "--split_window_q", "50", FASTQ)
    assert p.returncode == 1 and p.stderr == b"Error: --trim_adapters cannot be used with --split_window_q\n"
    p = run(exe, *bad, "--exclude_k", "20", FASTQ)
    assert p.returncode == 1 and p.stderr == b"Error: --exclude_k needs --exclude\n"
    p = run(exe, *bad, "--max_low_complexity", "0", FASTQ)
    assert p.returncode == 1 and p.stderr == b"Error: the value for --max_low_complexity must be greater than 0 and at most 100\n"
    p = run(exe, *bad, "--low_complexity_score", "20", FASTQ)
    assert p.returncode == 1 and p.stderr == b"Error: --low_complexity_score needs --max_low_complexity\n"
    p = run(exe, *bad, "--trim_adapters", FASTA, "--adapter_overhang", "53", FASTQ)
    assert p.returncode == 1 and p.stderr == b"Error: the value for --adapter_overhang must be an integer between 0 and 52\n"
    p = run(exe, *bad, "--adapter_overhang", "10", FASTQ)
    assert p.returncode == 1 and p.stderr == b"Error: --adapter_overhang needs --trim_adapters\n"
    # ... and with those in order the flag's own answer
    p = run(exe, *bad, "--trim_adapters", FASTA, "--adapter_overhang", "10", "--max_low_complexity", "50", FASTQ)
    assert p.returncode == 1 and p.stdout == b"" and p.stderr == BAD_VALUE
    # the readers' own messages
    p = run(exe, "--trim_ends_q", "abc", FASTQ)
    assert p.returncode == 1 and p.stderr == b"Error: argument 'float' received invalid value type 'abc'\n"
    p = run(exe, "--trim_ends_q", "-5", FASTQ)
    assert p.returncode == 1 and p.stderr == b"Error: argument 'float' received invalid value type '-5'\n"
    p = run(exe, FASTQ, "--trim_ends_q")
    assert p.returncode == 1 and p.stderr == b"Error: flag 'trim_ends_q' requires an argument but received none\n"


def test_the_flag_alone_is_a_threshold(exe):
    p = run(exe, FASTQ)
    assert p.returncode == 1 and p.stderr == NO_THRESHOLDS
    assert accepted(exe, "--trim_ends_q", "90", FASTQ)
    # with every mode it is meant to work with: the arguments are accepted
    assert accepted(exe, "--trim_ends_q", "90", "--min_length", "1000", "--gzip", "--verbose", "--gpus", "2", FASTQ)
    assert accepted(exe, "--trim_ends_q", "90", "--exclude", FASTA, "--exclude_k", "21", "--bam", "--keep_percent", "70", FASTQ)
    assert accepted(exe, "--trim_ends_q", "90", "--max_low_complexity", "50", "--report", os.devnull, FASTQ)


def test_help_is_the_reference_menu(exe):
    p = run(exe, "--help")
    assert p.returncode == 0 and b"trim_ends" not in p.stderr and b"--min_window_q [float]" in p.stderr
    q = run(exe, "--trim_ends_q", "90", "--help")
    assert q.returncode == 0 and q.stderr == p.stderr and q.stdout == p.stdout
