"""--split_window_q on the command line, as far as it goes without a GPU: arguments are judged before any device is asked for.
The flag's two errors come behind every check of the reference (status 1, nothing on stdout), the flag alone counts as a threshold,
and --help stays the reference's menu."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "filtlong_amd", "bin", "filtlong")
FASTQ = os.path.join(ROOT, "tests", "golden", "ref_fixtures", "test_sort.fastq")
NO_THRESHOLDS = b"Error: no thresholds set, you must use one of the following options:\ntarget_bases, keep_percent, min_length, max_length, min_mean_q, min_window_q, trim, split\n"


@pytest.fixture(scope="module")
def exe():
    if not os.path.exists(EXE):
        import __graft_entry__
        __graft_entry__.build()
    return EXE


def run(exe, *args, env=None):
    return subprocess.run([exe] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)


@pytest.mark.parametrize("value", ["0", "100", "100.5", "0.0"])
def test_value_out_of_range(exe, value):
    p = run(exe, "--split_window_q", value, FASTQ)
    assert p.returncode == 1 and p.stdout == b""
    assert p.stderr == b"Error: the value for --split_window_q must be greater than 0 and less than 100\n"


@pytest.mark.parametrize("ref", [["-a"], ["-1"], ["-2"], ["-1", "-2"], ["--assembly"]])
def test_not_with_an_external_reference(exe, ref):
    args = []
    for flag in ref:
        args += [flag, FASTQ]
    p = run(exe, "--split_window_q", "85", *args, FASTQ)
    assert p.returncode == 1 and p.stdout == b""
    assert p.stderr == b"Error: --split_window_q cannot be used with an external reference\n"


def test_the_new_checks_come_last(exe):
    # every message of the reference wins over the flag's own
    p = run(exe, "--split_window_q", "0", "--min_length", "0", FASTQ)
    assert p.returncode == 1 and p.stderr == b"Error: the value for --min_length must be a positive integer\n"
    p = run(exe, "--split_window_q", "0", "--window_size", "0", FASTQ)
    assert p.returncode == 1 and p.stderr == b"Error: the value for --window_size must be a positive integer\n"
    p = run(exe, "--split_window_q", "0", "--gzip", "--bam", FASTQ)
    assert p.returncode == 1 and p.stderr == b"Error: --gzip and --bam cannot be used together\n"
    p = run(exe, "--split_window_q", "85", "--trim", FASTQ)
    assert p.returncode == 1 and p.stderr == b"Error: assembly or read reference is required to use --trim\n"
    p = run(exe, "--split_window_q", "85", FASTQ + ".missing")
    assert p.returncode == 1 and p.stderr.startswith(b"Error: cannot find file: ")
    p = run(exe, "--split_window_q", "abc", FASTQ)
    assert p.returncode == 1 and p.stderr == b"Error: argument 'float' received invalid value type 'abc'\n"
    p = run(exe, "--split_window_q")
    assert p.returncode == 1 and p.stderr == b"Error: flag 'split_window_q' requires an argument but received none\n"


def test_the_flag_alone_is_a_threshold(exe):
    p = run(exe, FASTQ)
    assert p.returncode == 1 and p.stderr == NO_THRESHOLDS
    # with the flag the arguments are accepted: the run goes on to the environment check, which answers before any device is asked for
    p = run(exe, "--split_window_q", "85", FASTQ, env=dict(os.environ, FLX_CLI_NO_SUCH_SWITCH="1"))
    assert p.returncode == 1 and p.stdout == b""
    assert p.stderr == b"Error: unknown environment variable FLX_CLI_NO_SUCH_SWITCH (the FLX_CLI_* switches are listed in README.md)\n"


def test_help_is_the_reference_menu(exe):
    p = run(exe, "--help")
    assert p.returncode == 0 and b"split_window_q" not in p.stderr and b"--min_window_q [float]" in p.stderr
