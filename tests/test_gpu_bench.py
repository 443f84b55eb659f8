"""bench.py as every build is measured and compared with it: a plain run times exactly --steps steps and reports nothing of
--full, and --dump-outputs writes what the timed path computed in its last step, the same in every run with the same
arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def run_bench(argv):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "FLX_RANK_SORT")}
    r = subprocess.run([sys.executable, BENCH] + argv, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    lines = [l for l in r.stdout.decode().splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def load_dir(d):
    files = sorted(os.listdir(d))
    assert all(f.endswith(".npy") for f in files) and sum(os.path.getsize(os.path.join(d, f)) for f in files) <= 64 << 20
    out = {f[:-4]: np.load(os.path.join(d, f)) for f in files}
    assert all(a.dtype in (np.float32, np.float64) for a in out.values())
    return out


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_dump_sample_is_fixed():
    sys.path.insert(0, ROOT)
    import bench
    n = bench.DUMP_SAMPLE * 3 + 7
    a, b = bench.dump_index(n), bench.dump_index(n)
    assert len(a) == bench.DUMP_SAMPLE and (a == b).all() and (np.diff(a) > 0).all() and 0 <= a[0] and a[-1] < n
    assert (bench.dump_index(1000) == np.arange(1000)).all()


@pytest.mark.gpu
def test_plain_run_dumps_the_last_steps_outputs(tmp_path, oracle):
    from filtlong_amd import synth
    n = 40_000
    runs = []
    for k in range(2):
        d = str(tmp_path / ("out%d" % k))
        j = run_bench(["--gpus", "1", "--steps", "3", "--warmup", "1", "--reads", str(n), "--dump-outputs", d,
                       "--dump-flags", str(tmp_path / ("flags%d" % k))])
        assert j["steps"] == 3 and j["warmup"] == 1 and j["ms_per_step"] > 0 and j["metric"] == "Mbases/s scored+sorted"
        assert not {"cpu_baseline", "extras", "verify"} & set(j), sorted(j)
        runs.append((j, load_dir(d)))
    (j, a), (_, b) = runs
    assert sorted(a) == ["cut", "mean_q", "passed", "read_index", "window_q"]
    assert all(same(a[k], b[k]) for k in a)
    assert (a["read_index"] == np.arange(n)).all()
    flags = np.load(str(tmp_path / "flags0") + ".rank0.npy")
    assert (a["passed"] == flags).all() and 0 < flags.sum() < n
    assert list(a["cut"]) == [j["cut"]["target_bases"], j["cut"]["kept_bases"], j["cut"]["outcome"], j["cut"]["audited"],
                              j["cut"]["exact_fallback"], int(flags.sum())]
    # the per-read values are the reads' own: bit for bit the oracle's on the same synthetic reads
    lens = synth.lengths(n)
    p = oracle.make_params()
    for i in range(0, n, 997):
        want = oracle.score_read(None, synth.qual_read(i, int(lens[i])).tobytes(), p)
        assert a["mean_q"][i] == want["mean_q"] and a["window_q"][i] == want["window_q"], i


@pytest.mark.gpu
def test_kmer_config_dumps_the_same_outputs_twice(tmp_path):
    n = 3000
    outs = []
    for k in range(2):
        d = str(tmp_path / ("out%d" % k))
        j = run_bench(["--config", "c3", "--steps", "2", "--warmup", "1", "--reads", str(n), "--dump-outputs", d])
        assert j["steps"] == 2 and j["ms_per_step"] > 0 and "cpu_baseline" not in j
        outs.append(load_dir(d))
    a, b = outs
    assert sorted(a) == ["cut", "first_covered", "last_covered", "read_index", "reads2_index", "reads2_length", "reads2_mean_q",
                         "reads2_passed", "reads2_window_q"]
    assert all(same(a[k], b[k]) for k in a)
    assert a["cut"][1] == j["cut"]["kept_bases"] and a["cut"][4] == len(a["reads2_index"]) == n
