"""The segment arithmetic of the coverage stage's cooperative path (filtlong_amd/csrc/cover_segments.h, shared by the cover kernels,
cover_long.hip and this simulation) restated on the host — tools/sim_cover_segments.cpp: brute-force coverage of random and
engineered byte streams against a random member set, and the same coverage stitched from the segments' virtual reads [S, T)
restricted to their emit ranges; identical bits, count, first and last for every length from 0 to 2000 and segment sizes of 32 ..
2048 bases in place of the kernels' P x 1024.  No GPU; the kernels themselves are held against the oracle in
tests/test_gpu_kmer_cover_long.py."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_stitched_segments_equal_the_whole_read(tmp_path):
    exe = str(tmp_path / "sim_cover_segments")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tools", "sim_cover_segments.cpp")])
    run = subprocess.run([exe, "2000"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    out = run.stdout.decode()
    m = re.search(r"exactness: (\d+) cases, (\d+) segments, (\d+) mismatches", out)
    assert run.returncode == 0 and m and int(m.group(3)) == 0, out[-2000:]
    # per segment size: every length once with islands and gaps, every seventh with text pieces, and the engineered streams
    assert int(m.group(1)) >= 6 * (2001 + 2001 // 7 + 9 * 2 * 7 * 60), out[-2000:]
    assert int(m.group(2)) > 5 * int(m.group(1)), out[-2000:]
