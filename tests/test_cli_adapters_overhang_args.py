"""--adapter_overhang on the command line, as far as it goes without a GPU: the two new argument errors come behind every existing
check, the --low_complexity_score ones included, in their order (status 1, nothing on stdout); 0 is accepted; the old messages are
unchanged; --help stays the reference's menu."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "filtlong_amd", "bin", "filtlong")
FASTQ = os.path.join(ROOT, "tests", "golden", "ref_fixtures", "test_sort.fastq")
FASTA = os.path.join(ROOT, "tests", "golden", "ref_fixtures", "test_reference.fasta")
BAD_OVERHANG = b"Error: the value for --adapter_overhang must be an integer between 0 and 52\n"
NEEDS_TRIM = b"Error: --adapter_overhang needs --trim_adapters\n"
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
    f = tmp_path_factory.mktemp("adapters_overhang_args") / "adapters.fa"
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


@pytest.mark.parametrize("value", ["53", "64", "100", "-1", "8.5", "abc", "", "1e1", "0x10", "1000000"])
def test_overhang_out_of_range(exe, adapters, value):
    assert refused(exe, BAD_OVERHANG, "--trim_adapters", adapters, "--adapter_overhang", value, FASTQ)


@pytest.mark.parametrize("value", ["0", "1", "8", "52", "008"])
def test_values_in_range(exe, adapters, value):
    assert accepted(exe, "--trim_adapters", adapters, "--adapter_overhang", value, FASTQ)
    assert accepted(exe, "--adapter_overhang", value, "--trim_adapters", adapters, "--split_adapters", FASTQ)


def test_the_order_of_the_two(exe, adapters):
    # 1 the value, 2 the flag without --trim_adapters (0 included: the flag was given)
    assert refused(exe, BAD_OVERHANG, "--adapter_overhang", "53", "--min_length", "5", FASTQ)
    assert refused(exe, NEEDS_TRIM, "--adapter_overhang", "8", "--min_length", "5", FASTQ)
    assert refused(exe, NEEDS_TRIM, "--adapter_overhang", "0", "--min_length", "5", FASTQ)
    assert refused(exe, b"Error: flag 'adapter_overhang' requires an argument but received none\n", FASTQ, "--trim_adapters", adapters,
                   "--adapter_overhang")


def test_the_new_checks_come_behind_every_other(exe, adapters):
    bad = ["--adapter_overhang", "99"]
    missing = adapters + ".missing"
    assert refused(exe, b"Error: cannot find file: " + missing.encode() + b"\n", *bad, "--trim_adapters", missing, FASTQ)
    assert refused(exe, b"Error: the value for --adapter_errors must be an integer between 0 and 40\n", *bad, "--trim_adapters", adapters,
                   "--adapter_errors", "99", FASTQ)
    assert refused(exe, b"Error: the value for --adapter_window must be between 1 and 1024\n", *bad, "--trim_adapters", adapters, "--adapter_window", "0", FASTQ)
    assert refused(exe, b"Error: --adapter_errors needs --trim_adapters\n", *bad, "--adapter_errors", "20", "--min_length", "5", FASTQ)
    assert refused(exe, b"Error: --trim_adapters cannot be used with an external reference\n", *bad, "--trim_adapters", adapters, "-a", FASTA, FASTQ)
    assert refused(exe, b"Error: --trim_adapters cannot be used with --split_window_q\n", *bad, "--trim_adapters", adapters, "--split_window_q", "85", FASTQ)
    assert refused(exe, b"Error: the value for --adapter_split_errors must be an integer between 0 and 40\n", *bad, "--trim_adapters", adapters,
                   "--split_adapters", "--adapter_split_errors", "99", FASTQ)
    assert refused(exe, b"Error: --split_adapters needs --trim_adapters\n", *bad, "--split_adapters", "--min_length", "5", FASTQ)
    assert refused(exe, b"Error: --adapter_split_errors needs --split_adapters\n", *bad, "--trim_adapters", adapters, "--adapter_split_errors", "10", FASTQ)
    assert refused(exe, b"Error: the value for --exclude_k must be an integer between 16 and 31\n", *bad, "--trim_adapters", adapters, "--exclude", FASTA,
                   "--exclude_k", "99", FASTQ)
    assert refused(exe, b"Error: --exclude_k needs --exclude\n", *bad, "--trim_adapters", adapters, "--exclude_k", "17", FASTQ)
    assert refused(exe, b"Error: the value for --max_low_complexity must be greater than 0 and at most 100\n", *bad, "--trim_adapters", adapters,
                   "--max_low_complexity", "0", FASTQ)
    assert refused(exe, b"Error: the value for --low_complexity_score must be an integer between 10 and 300\n", *bad, "--trim_adapters", adapters,
                   "--max_low_complexity", "50", "--low_complexity_score", "9", FASTQ)
    assert refused(exe, b"Error: --low_complexity_score needs --max_low_complexity\n", *bad, "--trim_adapters", adapters, "--low_complexity_score", "20", FASTQ)
    assert refused(exe, b"Error: --low_complexity_score needs --max_low_complexity\n", "--adapter_overhang", "8", "--low_complexity_score", "20",
                   "--min_length", "5", FASTQ)
    assert refused(exe, b"Error: the value for --min_length must be a positive integer\n", *bad, "--min_length", "0", FASTQ)


def test_the_flag_is_no_threshold_of_its_own(exe, adapters):
    no_thresholds = (b"Error: no thresholds set, you must use one of the following options:\n"
                     b"target_bases, keep_percent, min_length, max_length, min_mean_q, min_window_q, trim, split\n")
    assert refused(exe, no_thresholds, "--adapter_overhang", "8", FASTQ)
    assert accepted(exe, "--trim_adapters", adapters, "--adapter_overhang", "8", "--split_adapters", "--exclude", FASTA, "--exclude_k", "21",
                    "--max_low_complexity", "50", "--gzip", "--verbose", "--gpus", "2", FASTQ)
    assert accepted(exe, "--trim_adapters", adapters, "--adapter_overhang", "16", "--bam", "--keep_percent", "70", FASTQ)


def test_help_is_the_reference_menu(exe):
    p = run(exe, "--help")
    assert p.returncode == 0 and b"adapter" not in p.stderr and b"overhang" not in p.stderr and b"--min_window_q [float]" in p.stderr
