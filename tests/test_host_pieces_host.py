"""csrc/host_pieces.h without a GPU: the buffers a slot owns (grown alone and only when too small, reused, moved, freed once) and the
cut of a call into pieces of whole records, in tests/host_pieces_host.cpp, built with -O2 and again with the address and
undefined-behaviour sanitizers (a stand-alone program on stubs of the allocation calls: no preload, no Python, no GPU)."""
import os
import subprocess

import pytest

from test_bam_host import BUILDS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_owned_buffers_and_piece_cutter(build, tmp_path):
    exe = str(tmp_path / "host_pieces_host")
    subprocess.check_call(["g++", "-std=c++17", "-Wall"] + BUILDS[build] + ["-I" + os.path.join(ROOT, "filtlong_amd", "csrc"), "-o", exe,
                                                                           os.path.join(ROOT, "tests", "host_pieces_host.cpp")])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0 and p.stdout == b"ok\n", p.stderr.decode()[-3000:]
