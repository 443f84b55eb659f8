"""--trim_adapters / --adapter_errors / --adapter_window on the command line, as far as it goes without a GPU: the six argument errors
come behind every check of the reference, of --split_window_q and of --exclude, in their order (status 1, nothing on stdout), and the
missing FILE is found before any device is asked for; the flag alone counts as a threshold; --help stays the reference's menu.  The
two messages about the file's contents need no device either: the file is read in front of the first use of one."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "filtlong_amd", "bin", "filtlong")
FASTQ = os.path.join(ROOT, "tests", "golden", "ref_fixtures", "test_sort.fastq")
FASTA = os.path.join(ROOT, "tests", "golden", "ref_fixtures", "test_reference.fasta")
NO_THRESHOLDS = b"Error: no thresholds set, you must use one of the following options:\ntarget_bases, keep_percent, min_length, max_length, min_mean_q, min_window_q, trim, split\n"
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
    f = tmp_path_factory.mktemp("adapters_args") / "adapters.fa"
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


def test_missing_file(exe, adapters):
    assert refused(exe, b"Error: cannot find file: " + (adapters + ".missing").encode() + b"\n", "--trim_adapters", adapters + ".missing", FASTQ)


@pytest.mark.parametrize("value", ["41", "100", "-1", "20.5", "abc", "", "1e1", "0x10", "1000000"])
def test_errors_out_of_range(exe, adapters, value):
    assert refused(exe, BAD_ERRORS, "--trim_adapters", adapters, "--adapter_errors", value, FASTQ)


@pytest.mark.parametrize("value", ["0", "1025", "-3", "150.0", "wide", "9999999"])
def test_window_out_of_range(exe, adapters, value):
    assert refused(exe, BAD_WINDOW, "--trim_adapters", adapters, "--adapter_window", value, FASTQ)


@pytest.mark.parametrize("errors,window", [("0", "1"), ("40", "1024"), ("20", "150"), ("007", "0150")])
def test_values_in_range(exe, adapters, errors, window):
    assert accepted(exe, "--trim_adapters", adapters, "--adapter_errors", errors, "--adapter_window", window, FASTQ)


def test_the_order_of_the_six(exe, adapters):
    missing = adapters + ".missing"
    # 1 the file, 2 the errors, 3 the window, 4 a value without the flag, 5 an external reference, 6 --split_window_q
    assert refused(exe, b"Error: cannot find file: " + missing.encode() + b"\n", "--trim_adapters", missing, "--adapter_errors", "99", "--adapter_window", "0",
                   "-a", FASTA, FASTQ)
    assert refused(exe, BAD_ERRORS, "--trim_adapters", adapters, "--adapter_errors", "99", "--adapter_window", "0", "-a", FASTA, FASTQ)
    assert refused(exe, BAD_WINDOW, "--trim_adapters", adapters, "--adapter_errors", "20", "--adapter_window", "0", "-a", FASTA, FASTQ)
    assert refused(exe, BAD_ERRORS, "--adapter_errors", "99", "--adapter_window", "0", "--min_length", "5", FASTQ)
    assert refused(exe, BAD_WINDOW, "--adapter_window", "0", "--min_length", "5", FASTQ)
    assert refused(exe, b"Error: --adapter_errors needs --trim_adapters\n", "--adapter_errors", "20", "--adapter_window", "100", "--min_length", "5", FASTQ)
    assert refused(exe, b"Error: --adapter_window needs --trim_adapters\n", "--adapter_window", "100", "--min_length", "5", FASTQ)
    assert refused(exe, b"Error: --adapter_errors needs --trim_adapters\n", "--adapter_errors", "20", "-a", FASTA, "--trim", FASTQ)
    external = b"Error: --trim_adapters cannot be used with an external reference\n"
    assert refused(exe, external, "--trim_adapters", adapters, "-a", FASTA, FASTQ)
    assert refused(exe, external, "--trim_adapters", adapters, "-1", FASTQ, "--trim", FASTQ)
    assert refused(exe, b"Error: --trim_adapters cannot be used with --split_window_q\n", "--trim_adapters", adapters, "--split_window_q", "85", FASTQ)
    assert refused(exe, b"Error: --split_window_q cannot be used with an external reference\n", "--trim_adapters", adapters, "--split_window_q", "85", "-a", FASTA, FASTQ)


def test_the_new_checks_come_last(exe, adapters):
    bad = ["--trim_adapters", adapters + ".missing", "--adapter_errors", "99", "--adapter_window", "0"]
    assert refused(exe, b"Error: the value for --min_length must be a positive integer\n", *bad, "--min_length", "0", FASTQ)
    assert refused(exe, b"Error: the value for --window_size must be a positive integer\n", *bad, "--window_size", "0", FASTQ)
    assert refused(exe, b"Error: the value for --keep_percent must be greater than 0 and less than 100\n", *bad, "--keep_percent", "100", FASTQ)
    assert refused(exe, b"Error: --gzip and --bam cannot be used together\n", *bad, "--gzip", "--bam", FASTQ)
    assert refused(exe, b"Error: assembly or read reference is required to use --trim\n", *bad, "--trim", FASTQ)
    assert refused(exe, b"Error: cannot find file: " + (FASTQ + ".missing").encode() + b"\n", *bad, FASTQ + ".missing")
    assert refused(exe, b"Error: the value for --split_window_q must be greater than 0 and less than 100\n", *bad, "--split_window_q", "0", FASTQ)
    # ... and those of --exclude
    assert refused(exe, b"Error: cannot find file: " + (FASTA + ".missing").encode() + b"\n", *bad, "--exclude", FASTA + ".missing", FASTQ)
    assert refused(exe, b"Error: the value for --exclude_percent must be greater than 0 and at most 100\n", *bad, "--exclude", FASTA, "--exclude_percent", "0", FASTQ)
    assert refused(exe, b"Error: --exclude_percent needs --exclude\n", *bad, "--exclude_percent", "5", FASTQ)
    # the readers' own messages
    assert refused(exe, b"Error: flag 'trim_adapters' requires an argument but received none\n", FASTQ, "--trim_adapters")
    assert refused(exe, b"Error: flag 'adapter_errors' requires an argument but received none\n", FASTQ, "--trim_adapters", adapters, "--adapter_errors")
    assert refused(exe, b"Error: flag 'adapter_window' requires an argument but received none\n", FASTQ, "--trim_adapters", adapters, "--adapter_window")


def test_the_flag_alone_is_a_threshold(exe, adapters):
    assert refused(exe, NO_THRESHOLDS, FASTQ)
    assert accepted(exe, "--trim_adapters", adapters, FASTQ)
    assert accepted(exe, "--trim_adapters", adapters, "--exclude", FASTA, "--gzip", "--verbose", "--gpus", "2", FASTQ)
    assert accepted(exe, "--trim_adapters", adapters, "--bam", "--keep_percent", "70", FASTQ)


def test_report_file_must_not_be_the_adapter_file(exe, adapters):
    assert refused(exe, b"Error: report file is one of the input files: " + adapters.encode() + b"\n", "--trim_adapters", adapters, "--report", adapters, FASTQ)
    assert open(adapters, "rb").read() == TWO


@pytest.mark.parametrize("text,message", [
    (b">short\nACGTACGTACG\n", b"Error: adapter short must have 12 to 64 bases of ACGT\n"),
    (TWO + b">long one\n" + b"ACGT" * 16 + b"A\n", b"Error: adapter long must have 12 to 64 bases of ACGT\n"),
    (TWO + b">with_n\nACGTACGTNACGTACGT\n", b"Error: adapter with_n must have 12 to 64 bases of ACGT\n"),
    (b">iupac\nACGTACGTRACGTACGT\n" + b">x\nAC\n" * 200, b"Error: adapter iupac must have 12 to 64 bases of ACGT\n"),
    (b"", b"Error: the file for --trim_adapters holds no sequence\n"),
    (b"".join(b">a%d\nACGTACGTACGTAC\n" % i for i in range(129)), b"Error: the file for --trim_adapters holds more than 128 sequences\n"),
])
def test_what_the_file_may_hold(exe, tmp_path, text, message):
    f = tmp_path / "a.fa"
    f.write_bytes(text)
    p = run(exe, "--trim_adapters", str(f), FASTQ)
    assert p.returncode == 1 and p.stdout == b""
    assert p.stderr.startswith(b"\nReading adapters\n  " + str(f).encode() + b"\n") and p.stderr.endswith(b"\n\n" + message)


def test_help_is_the_reference_menu(exe):
    p = run(exe, "--help")
    assert p.returncode == 0 and b"adapter" not in p.stderr and b"--min_window_q [float]" in p.stderr
