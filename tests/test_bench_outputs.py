"""bench.py's plain run, --full and --dump-outputs: what the line of a plain run holds, that the dumped arrays are the last timed step's outputs with the unwritten tails
masked, and that the same arguments give the same arrays."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("cpu_baseline", "cpu_baseline_all_cores", "host_inclusive", "general_path", "with_YP_final", "predicted_scaling", "ensemble_run")


def _fake_ensemble(n, mp, N, thermal, seed=1):
    """what dump_outputs reads of an EnsembleSolution of a device=True call: torch tensors whose rows are garbage beyond n_pts"""
    import torch
    rng = np.random.default_rng(seed)
    n_pts = rng.integers(1, mp + 1, n).astype(np.int32)
    e = types.SimpleNamespace()
    for nm in ("t", "V", "I", "SOC"):
        setattr(e, nm, torch.from_numpy(rng.random((n, mp)) + 1.0))
    e.T_avg = torch.from_numpy(rng.random((n, mp)) + 1.0) if thermal else None
    e.n_pts = torch.from_numpy(n_pts)
    e.Y = torch.from_numpy(rng.random((n, N)))
    e.run_info = np.zeros((n, 2), dtype=[("flag", np.int32), ("t_end", np.float64)])
    e.run_info["flag"] = 3
    e.run_info["t_end"] = rng.random((n, 2))
    e.counters = np.zeros(n, dtype=[("n_steps", np.int64), ("n_newton", np.int64)])
    e.counters["n_steps"] = n_pts - 1
    return e, n_pts


def test_dump_outputs_masks_the_unwritten_tail_and_keeps_every_cell_that_fits(tmp_path):
    import bench
    e, n_pts = _fake_ensemble(50, 16, 7, thermal=True)
    bench.dump_outputs(e, str(tmp_path / "d"))
    got = {f[:-4]: np.load(tmp_path / "d" / f) for f in os.listdir(tmp_path / "d")}
    assert sorted(got) == sorted(["t", "V", "I", "SOC", "T_avg", "Y_final", "n_pts", "flag", "t_end", "n_steps", "n_newton", "cells"])
    assert all(a.dtype == np.float64 for a in got.values())
    assert np.array_equal(got["cells"], np.arange(50)) and np.array_equal(got["n_pts"], n_pts) and np.array_equal(got["Y_final"], e.Y.numpy())
    saved = np.arange(16)[None, :] < n_pts[:, None]
    for nm in ("t", "V", "I", "SOC", "T_avg"):
        assert np.array_equal(got[nm][saved], getattr(e, nm).numpy()[saved]) and (got[nm][~saved] == 0.0).all()
    assert np.array_equal(got["t_end"], e.run_info["t_end"]) and (got["flag"] == 3).all()


def test_dump_outputs_takes_the_same_sample_of_a_large_output_every_time(tmp_path, monkeypatch):
    import bench
    e, n_pts = _fake_ensemble(400, 32, 11, thermal=False)
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 100 * 8 * (4 * 32 + 11 + 2 * 2 + 4))       # room for 100 of the 400 cells
    bench.dump_outputs(e, str(tmp_path / "a"))
    bench.dump_outputs(e, str(tmp_path / "b"))
    cells = np.load(tmp_path / "a" / "cells.npy").astype(int)
    assert cells.shape == (100,) and (np.diff(cells) > 0).all() and cells.max() < 400
    for f in os.listdir(tmp_path / "a"):
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)), f
    assert np.array_equal(np.load(tmp_path / "a" / "Y_final.npy"), e.Y.numpy()[cells])
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) < 64 << 20


def _bench(*args):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + list(args), capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_is_lean_and_two_runs_dump_the_same_outputs(hip_model, tmp_path):
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    d = _bench("--steps", "7", "--warmup", "2", "--dump-outputs", a)
    _bench("--steps", "3", "--warmup", "1", "--dump-outputs", b)
    assert d["steps"] == 7 and d["warmup"] == 2 and d["value"] > 0 and d["unit"] == "trajectories/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
    assert abs(d["ms_per_step"] * 1e-3 * d["value"] - 1024) < 1e-6 * 1024            # value = cells per timed step / seconds per timed step
    assert not [k for k in FULL_ONLY if k in d] and "measured_copy_peak" not in d["roofline"]
    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b)) and "V.npy" in names and "Y_final.npy" in names
    for f in names:
        x = np.load(os.path.join(a, f))
        assert x.dtype == np.float64 and x.shape[0] == 1024 and np.isfinite(x).all(), f
        assert np.array_equal(x, np.load(os.path.join(b, f))), f
    n_pts = np.load(os.path.join(a, "n_pts.npy")).astype(int)
    V, t = np.load(os.path.join(a, "V.npy")), np.load(os.path.join(a, "t.npy"))
    assert (n_pts > 1).all() and (V[np.arange(1024), n_pts - 1] > 2.0).all() and np.abs(t[np.arange(1024), n_pts - 1] - 3600.0).max() < 1e-5 and (V[:, n_pts.max():] == 0.0).all()


@pytest.mark.gpu
def test_full_run_carries_everything_the_plain_run_left_out(hip_model):
    d = _bench("--steps", "3", "--warmup", "1", "--full", "--cpu-seconds", "2")
    for k in ("cpu_baseline", "cpu_baseline_all_cores", "host_inclusive", "general_path", "with_YP_final"):
        assert k in d, k
    assert d["roofline"]["measured_copy_peak"] > 0 and d["steps"] == 3 and d["ms_per_step"] > 0
