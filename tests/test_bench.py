"""bench.py's own options: --dump-outputs (what the timed path computed, as float64 .npy files), --steps, and the
plain run (the primary workload only; everything else behind --full)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

MAX_HASH = 18446744073709552


def _bench():
    sys.path.insert(0, ROOT)
    import bench
    return bench


def test_dump_outputs_small_sketch_is_written_whole(tmp_path):
    bench = _bench()
    mins = np.array([3, 70000, (1 << 53) + 1, MAX_HASH - 1], dtype=np.uint64)
    bench.dump_outputs(str(tmp_path), mins)
    assert sorted(os.listdir(tmp_path)) == ["mins.npy", "mins_low16.npy", "retained.npy"]
    for f in os.listdir(tmp_path):
        assert np.load(tmp_path / f).dtype == np.float64
    assert np.load(tmp_path / "retained.npy").tolist() == [4.0]
    assert np.load(tmp_path / "mins.npy").tolist() == [float(x) for x in mins.tolist()]
    # the low 16 bits are exact where float64 rounds the hash itself
    assert np.load(tmp_path / "mins_low16.npy").tolist() == [3.0, float(70000 & 0xFFFF), 1.0, float((MAX_HASH - 1) & 0xFFFF)]


def test_dump_outputs_large_sketch_is_a_fixed_sample_under_64_mb(tmp_path):
    bench = _bench()
    n = bench.DUMP_SAMPLE * 3 + 17
    mins = np.sort(np.random.default_rng(5).integers(0, MAX_HASH, size=n, dtype=np.uint64))
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(str(a), mins)
    bench.dump_outputs(str(b), mins.copy())
    assert sum(os.path.getsize(a / f) for f in os.listdir(a)) <= 64 << 20
    assert np.load(a / "retained.npy").tolist() == [float(n)]
    sample = np.load(a / "mins.npy")
    assert sample.shape == (bench.DUMP_SAMPLE,) and bool((sample[1:] >= sample[:-1]).all())
    for f in os.listdir(a):
        assert (np.load(a / f) == np.load(b / f)).all(), f
    # the sample is drawn from the sketch: every sampled low-16 value belongs to a hash that is in it
    low = np.load(a / "mins_low16.npy")
    assert low.shape == sample.shape and bool(np.isin(low, (mins & np.uint64(0xFFFF)).astype(np.float64)).all())


@pytest.mark.parametrize("argv", [["--steps", "0"], ["--warmup", "-1"]])
def test_bench_rejects_a_step_count_it_cannot_time(argv):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + argv, cwd=ROOT, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 2 and "--steps must be >= 1" in r.stderr


@pytest.mark.gpu
def test_plain_run_dumps_the_sketch_of_its_last_step(pkg, coracle, tmp_path):
    """A plain run times the primary workload only, and --dump-outputs holds the sketch its last timed step made:
    equal to the C oracle's sketch of the same seeded records."""
    n_rec = 6
    out = tmp_path / "out"
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--gb", str(n_rec / 1000.0), "--steps", "3", "--warmup", "1",
           "--dump-outputs", str(out)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["value"] > 0 and d["full"] is False
    assert d["unit"] == "k-mers/s" and d["higher_is_better"] is True and d["dtype"] == "u64"
    for key in ("protein", "compare", "cpu_baseline", "host_input", "union_across_ranks"):
        assert d[key] is None, key
    o = coracle.MinHash(0, 31, False, 42, MAX_HASH, False)
    for rec in range(n_rec):
        o.add_sequence(bytes(coracle.synth_dna(rec * 1000000, 1000000, 2, 0)), True)
    ref = o.mins_np()
    assert d["config"]["retained_hashes"] == ref.size
    assert np.load(out / "retained.npy").tolist() == [float(ref.size)]
    assert (np.load(out / "mins.npy") == ref.astype(np.float64)).all()
    assert (np.load(out / "mins_low16.npy") == (ref & np.uint64(0xFFFF)).astype(np.float64)).all()
