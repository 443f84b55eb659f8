"""The cooperative window fold of ultra-long reads in k-mer mode (filtlong_amd/csrc/score_kmer_long.hip) restated on the host —
tools/sim_fold_long.cpp, with the kernel's own grid table and start of a regime (filtlong_amd/csrc/fold_grid_tab.h): word summaries, 64 at a time, the first word that leaves the regime replayed in floating point, the rest
tested again — against the plain recurrence of the reference (src/read.cpp:216-236 with qualities 0.0 / 1.0), bit for bit in w and
mn.  Random and engineered bit streams (the clean / junk periods of tests/test_gpu_kmer.py::test_integer_grid_folds_vs_oracle,
all-zero and all-one streams, lengths ws-1 .. ws+1, 1023 .. 1025, 2047 .. 2049), as a read of its own and as a child at a bit offset
inside a longer row, for window sizes 8, 64, 128, 250, 500, 333 and 2047.  No GPU; the kernel itself is held against the oracle in
tests/test_gpu_kmer_long.py."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_chunked_walk_equals_the_plain_recurrence(tmp_path):
    exe = str(tmp_path / "sim_fold_long")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", exe, os.path.join(ROOT, "tools", "sim_fold_long.cpp")])
    run = subprocess.run([exe, "300"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    out = run.stdout.decode()
    m = re.search(r"exactness: (\d+) cases, (\d+) mismatches", out)
    assert run.returncode == 0 and m and int(m.group(2)) == 0, out[-2000:]
    # per window size: 60 period streams, 60 length streams (less those shorter than the window: at least 40) and 300 random ones, each twice
    assert int(m.group(1)) >= 7 * 2 * (60 + 40 + 300), out[-2000:]
    for ws in (8, 64, 128, 250, 500, 333, 2047):
        r = re.search(r"ws %d \(.*\): (\d+) words, (\d+) replayed" % ws, out)
        assert r and int(r.group(1)) > 100_000, (ws, out[-2000:])
    # the default window replays a small share of its words, a window without a paying regime many of them
    share = {ws: int(b) / int(a) for ws, a, b in re.findall(r"ws (\d+) \(.*\): (\d+) words, (\d+) replayed", out)}
    assert share["250"] < 0.1 and share["500"] < 0.1, share
