"""`--report FILE` on the command line and the host side of flx_summary's radix selection, without a GPU: the flag's argument
errors (raised before any GPU work, behind every check of the reference), and filtlong_amd/csrc/summary_select.h driven by
tests/summary_select_host.cpp under AddressSanitizer and UBSan against a sort.  The kernels are held against numpy in
tests/test_gpu_summary.py, the report itself in tests/test_gpu_report_cli.py."""
import os
import re
import subprocess

import pytest

import _cases
from test_cli_args import CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "filtlong_amd", "bin", "filtlong")
INPUT = os.path.join(_cases.FIXTURES, "test_sort.fastq")
ASM = os.path.join(_cases.FIXTURES, "test_reference.fasta")


@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.path.exists(BIN):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "filtlong_amd", "csrc"), "-s", "-j8"])
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "filtlong_amd", "cli"), "-s"])


def run(*args):
    p = subprocess.run([BIN] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, LANG="C", LC_ALL="C"))
    return p.returncode, p.stdout, p.stderr.decode()


def test_report_needs_a_value():
    for argv in (["--report"], ["--target_bases", "1000", INPUT, "--report"]):
        rc, out, err = run(*argv)
        assert rc == 1 and out == b"" and err == "Error: flag 'report' requires an argument but received none\n", err


def test_report_file_that_cannot_be_written(tmp_path):
    path = str(tmp_path / "no_such_directory" / "report.json")
    rc, out, err = run("--target_bases", "1000", "--report", path, INPUT)
    assert rc == 1 and out == b"" and err == "Error: cannot write report file: %s\n" % path, err
    assert not os.path.exists(path)


@pytest.mark.parametrize("argv,msg", CASES)
def test_reference_errors_come_first(tmp_path, argv, msg):
    """Every argument error of the reference is reported as before — same stderr, same status — when --report is there too, even
    one that cannot be written; and a report file that can is not created by a command line the reference refuses."""
    argv = [INPUT if a == "INPUT" else ASM if a == "ASSEMBLY" else a for a in argv]
    plain = run(*argv)
    assert plain[0] == 1 and msg in plain[2]
    bad = str(tmp_path / "no_such_directory" / "report.json")
    good = str(tmp_path / "report.json")
    assert run("--report", bad, *argv) == plain
    assert run(*(argv + ["--report", good])) == plain
    assert not os.path.exists(good)


def test_report_file_exists_once_the_arguments_are_good(tmp_path):
    """Once the arguments are good the file exists and its old content is gone; the rest of the surface is that of the run without
    the flag.  (Without a GPU the run then ends at the context and the file stays empty; what a run that succeeds writes is held
    in tests/test_gpu_report_cli.py.)"""
    path = tmp_path / "report.json"
    path.write_text("stale")
    rc, out, err = run("--target_bases", "1000", "--report", str(path), INPUT)
    assert path.exists() and b"stale" not in path.read_bytes()
    if rc != 0:
        assert path.read_bytes() == b""
    assert run("--target_bases", "1000", INPUT) == (rc, out, err)


def test_report_file_is_left_alone_by_a_run_the_environment_check_refuses(tmp_path):
    path = tmp_path / "report.json"
    path.write_text("earlier report")
    p = subprocess.run([BIN, "--target_bases", "1000", "--report", str(path), INPUT], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       env=dict(os.environ, LANG="C", LC_ALL="C", FLX_CLI_NO_SUCH_SWITCH="1"))
    assert p.returncode == 1 and b"unknown environment variable FLX_CLI_NO_SUCH_SWITCH" in p.stderr
    assert path.read_text() == "earlier report"


def test_report_file_must_not_be_an_input(tmp_path):
    reads = tmp_path / "reads.fastq"
    reads.write_bytes(open(INPUT, "rb").read())
    asm = tmp_path / "asm.fasta"
    asm.write_bytes(open(ASM, "rb").read())
    link = tmp_path / "link.fastq"
    os.symlink(str(reads), str(link))
    for report, argv in ((reads, ["--target_bases", "1000", str(reads)]), (link, ["--target_bases", "1000", str(reads)]),
                         (asm, ["-a", str(asm), "--target_bases", "1000", str(reads)])):
        rc, out, err = run("--report", str(report), *argv)
        assert rc == 1 and out == b"" and err == "Error: report file is one of the input files: %s\n" % report, err
    assert reads.read_bytes() == open(INPUT, "rb").read() and asm.read_bytes() == open(ASM, "rb").read()


def test_help_does_not_mention_the_flag():
    rc, out, err = run("--help")
    assert rc == 0 and "report" not in err and "gzip" not in err


def test_select_host_against_a_sort(tmp_path):
    exe = str(tmp_path / "summary_select_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tests", "summary_select_host.cpp")])
    p = subprocess.run([exe, "300"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    out = p.stdout.decode()
    m = re.search(r"select: (\d+) cases, (\d+) mismatches, (\d+) passes with shared rows", out)
    assert p.returncode == 0 and m and int(m.group(2)) == 0, out[-3000:]
    assert int(m.group(1)) >= 3 * (300 + 15) and int(m.group(3)) > 0, out[-500:]
