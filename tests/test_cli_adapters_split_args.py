"""--split_adapters / --adapter_split_errors on the command line, as far as it goes without a GPU: the three new argument errors come
behind every existing adapter check, in their order (status 1, nothing on stdout); the old messages are unchanged; --help stays the
reference's menu."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "filtlong_amd", "bin", "filtlong")
FASTQ = os.path.join(ROOT, "tests", "golden", "ref_fixtures", "test_sort.fastq")
FASTA = os.path.join(ROOT, "tests", "golden", "ref_fixtures", "test_reference.fasta")
NO_THRESHOLDS = b"Error: no thresholds set, you must use one of the following options:\ntarget_bases, keep_percent, min_length, max_length, min_mean_q, min_window_q, trim, split\n"
BAD_SPLIT_ERRORS =b"Error: the value for --adapter_split_errors must be an integer between 0 and 40\n"
NEEDS_TRIM = b"Error: --split_adapters needs --trim_adapters\n"
NEEDS_SPLIT = b"Error: --adapter_split_errors needs --split_adapters\n"
BAD_ERRORS = b"Error: the value for --adapter_errors must be an integer between 0 and 40\n"
BAD_WINDOW = b"Error: the value for --adapter_window must be between 1 and 1024\n"
ENV_ANSWER = b"Error: unknown environment variable FLX_CLI_NO_SUCH_SWITCH (the FLX_CLI_* switches are listed in README.md)\n"
TWO = b">ligation top\nAATGTACTTCGTTCAGTTACGTATTGCT\n>ligation_bottom\nGCAATACGTAACTGAACGAAGT\n"


@pytest.fixture(scope="module")
def exe():
    if not os.path.exists(EXE):
        import __graft_entry__
        __graft_entry__.build()
    return EXE


@pytest.fixture(scope="module")
def adapters(tmp_path_factory):
    f = tmp_path_factory.mktemp("adapters_split_args") / "adapters.fa"
    f.write_bytes(TWO)
    return str(f)


def run(exe, *args, env=None):
    return subprocess.run([exe] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)


def accepted(exe, *args):
    """the arguments pass: the run goes on to the environment check, which answers before any device is asked for"""
    p = run(exe, *args, env=dict(os.environ, FLX_CLI_NO_SUCH_SWITCH="1"))
    return p.returncode == 1 and p.stdout == b"" and p.stderr == ENV_ANSWER


def refused(exe, message, *args):
    p = run(exe, *args)
    return p.returncode == 1 and p.stdout == b"" and p.stderr == message


@pytest.mark.parametrize("value", ["41", "100", "-1", "10.5", "abc", "", "1e1", "0x10", "1000000"])
def test_split_errors_out_of_range(exe, adapters, value):
    assert refused(exe, BAD_SPLIT_ERRORS, "--trim_adapters", adapters, "--split_adapters", "--adapter_split_errors", value, FASTQ)


@pytest.mark.parametrize("value", ["0", "10", "40", "007"])
def test_values_in_range(exe, adapters, value):
    assert accepted(exe, "--trim_adapters", adapters, "--split_adapters", "--adapter_split_errors", value, FASTQ)
    assert accepted(exe, "--split_adapters", "--trim_adapters", adapters, FASTQ)


def test_the_order_of_the_three(exe, adapters):
    # 1 the value, 2 --split_adapters without --trim_adapters, 3 the value without --split_adapters
    assert refused(exe, BAD_SPLIT_ERRORS, "--split_adapters", "--adapter_split_errors", "99", "--min_length", "5", FASTQ)
    assert refused(exe, BAD_SPLIT_ERRORS, "--adapter_split_errors", "99", "--min_length", "5", FASTQ)
    assert refused(exe, NEEDS_TRIM, "--split_adapters", "--adapter_split_errors", "10", "--min_length", "5", FASTQ)
    assert refused(exe, NO_THRESHOLDS, "--split_adapters", FASTQ)  # (the flag is no threshold of its own: the reference's check is first)
    assert refused(exe, NEEDS_SPLIT, "--adapter_split_errors", "10", "--min_length", "5", FASTQ)
    assert refused(exe, NEEDS_SPLIT, "--trim_adapters", adapters, "--adapter_split_errors", "10", FASTQ)
    assert refused(exe, b"Error: flag 'adapter_split_errors' requires an argument but received none\n", FASTQ, "--trim_adapters", adapters,
                   "--split_adapters", "--adapter_split_errors")


def test_the_new_checks_come_behind_the_adapter_checks(exe, adapters):
    bad = ["--split_adapters", "--adapter_split_errors", "99"]
    missing = adapters + ".missing"
    assert refused(exe, b"Error: cannot find file: " + missing.encode() + b"\n", *bad, "--trim_adapters", missing, FASTQ)
    assert refused(exe, BAD_ERRORS, *bad, "--trim_adapters", adapters, "--adapter_errors", "99", FASTQ)
    assert refused(exe, BAD_WINDOW, *bad, "--trim_adapters", adapters, "--adapter_window", "0", FASTQ)
    assert refused(exe, b"Error: --adapter_errors needs --trim_adapters\n", *bad, "--adapter_errors", "20", "--min_length", "5", FASTQ)
    assert refused(exe, b"Error: --adapter_window needs --trim_adapters\n", *bad, "--adapter_window", "100", "--min_length", "5", FASTQ)
    assert refused(exe, b"Error: --trim_adapters cannot be used with an external reference\n", *bad, "--trim_adapters", adapters, "-a", FASTA, FASTQ)
    assert refused(exe, b"Error: --trim_adapters cannot be used with --split_window_q\n", *bad, "--trim_adapters", adapters, "--split_window_q", "85", FASTQ)
    assert refused(exe, b"Error: the value for --min_length must be a positive integer\n", *bad, "--min_length", "0", FASTQ)
    assert refused(exe, b"Error: --exclude_percent needs --exclude\n", *bad, "--exclude_percent", "5", "--min_length", "5", FASTQ)


def test_the_flag_is_no_threshold_of_its_own(exe, adapters):
    assert refused(exe, NEEDS_TRIM, "--split_adapters", "--min_length", "5", FASTQ)
    assert accepted(exe, "--trim_adapters", adapters, "--split_adapters", "--exclude", FASTA, "--gzip", "--verbose", "--gpus", "2", FASTQ)
    assert accepted(exe, "--trim_adapters", adapters, "--split_adapters", "--bam", "--keep_percent", "70", FASTQ)


def test_help_is_the_reference_menu(exe):
    p = run(exe, "--help")
    assert p.returncode == 0 and b"adapter" not in p.stderr and b"--min_window_q [float]" in p.stderr
