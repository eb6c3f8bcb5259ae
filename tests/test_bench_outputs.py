"""bench.py's plain run and `--dump-outputs`: a plain run times exactly --steps steps and runs nothing beyond the headline; the
dump is what the last timed step computed, identical from run to run for the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_dump_outputs_writes_the_mask_as_float32(tmp_path):
    import torch
    v = torch.from_numpy(np.random.default_rng(3).integers(0, 2, size=1000).astype(np.uint8))
    bench.dump_outputs(str(tmp_path), v)
    got = np.load(tmp_path / "valid.npy")
    assert got.dtype == np.float32 and np.array_equal(got, v.numpy().astype(np.float32))
    assert not (tmp_path / "valid_index.npy").exists()


def test_dump_outputs_samples_a_large_mask_with_a_fixed_seed(tmp_path, monkeypatch):
    import torch
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 4 * 1000)
    monkeypatch.setattr(bench, "DUMP_SAMPLE", 100)
    v = torch.from_numpy(np.random.default_rng(4).integers(0, 2, size=5000).astype(np.uint8))
    runs = []
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), v)
        runs.append((np.load(tmp_path / d / "valid.npy"), np.load(tmp_path / d / "valid_index.npy")))
    (val, idx), (val2, idx2) = runs
    assert val.dtype == np.float32 and idx.dtype == np.float64 and len(val) == len(idx) == 100
    assert np.array_equal(idx, idx2) and np.array_equal(val, val2)
    assert np.all(np.diff(idx) > 0) and np.array_equal(val, v.numpy()[idx.astype(np.int64)].astype(np.float32))
    bench.dump_outputs(str(tmp_path / "a"), v[:10])          # a smaller mask into the same directory: no stale index left behind
    assert not (tmp_path / "a" / "valid_index.npy").exists()


def test_steps_below_one_is_an_error():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--steps" in r.stderr


@pytest.mark.gpu
def test_plain_run_is_lean_and_its_dump_is_reproducible(tmp_path):
    E, S, steps = 64, 64, 3
    outs = []
    for d in ("a", "b"):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1",
                            "--envs", str(E), "--samples", str(S), "--dump-outputs", str(tmp_path / d)],
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1, r.stdout
        outs.append(json.loads(lines[0]))
    h = outs[0]
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in h, k
    assert h["steps"] == steps and h["ms_per_step"] > 0 and h["value"] > 0 and h["dtype"] == "f64"
    assert h["full"] is False and h["full_record"] is None and h["cpu_baseline"] is None
    s = h["summary"]
    assert s["planner"]["ms_per_batch"] is None and s["ik_solves_per_s"] is None and s["rollout_agent_steps_per_s"] == {}
    a, b = np.load(tmp_path / "a" / "valid.npy"), np.load(tmp_path / "b" / "valid.npy")
    assert a.dtype == np.float32 and a.shape == (E * S,) and set(np.unique(a)) <= {0.0, 1.0}
    assert np.array_equal(a, b)
    assert abs(float(a.mean()) - h["valid_fraction"]) < 1e-6
