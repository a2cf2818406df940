"""bench.py's command line: a plain run prints the headline only, --full the extra objects, and --dump-outputs writes what the
last timed step returned, the same from run to run for the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench as B  # noqa: E402

HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


def _last(P, W, H, seed=0):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    return {"color": r(3, H, W), "depth": r(1, H, W), "uncertainty": r(1, H, W), "radii": torch.randint(0, 9, (P,), dtype=torch.int32),
            "grad_means3D": r(P, 3), "grad_opacities": r(P, 1), "grad_uncertainties": r(P, 1), "grad_colors": r(P, 3),
            "grad_scales": r(P, 3), "grad_rotations": r(P, 4), "grad_means2D": r(P, 3)}


def test_dump_outputs_writes_every_array_whole_when_it_fits(tmp_path):
    P, W, H = 1000, 40, 24
    last = _last(P, W, H)
    B.dump_outputs(str(tmp_path), last, P)
    assert sorted(os.listdir(tmp_path)) == sorted([k + ".npy" for k in last] + ["gaussian_index.npy"])
    for k, v in last.items():
        a = np.load(tmp_path / (k + ".npy"))
        assert a.dtype == np.float32 and a.shape == tuple(v.shape)
        assert np.array_equal(a, v.float().numpy())
    assert np.array_equal(np.load(tmp_path / "gaussian_index.npy"), np.arange(P, dtype=np.float64))


def test_dump_outputs_samples_the_same_rows_within_the_budget(tmp_path, monkeypatch):
    P, W, H = 20_000, 40, 24
    monkeypatch.setattr(B, "DUMP_BUDGET_BYTES", 400_000)
    last = _last(P, W, H)
    for d in ("a", "b"):
        B.dump_outputs(str(tmp_path / d), last, P)
    files = sorted(os.listdir(tmp_path / "a"))
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 400_000 + 128 * len(files)  # (+ the npy headers)
    idx = np.load(tmp_path / "a" / "gaussian_index.npy")
    assert idx.dtype == np.float64 and 0 < len(idx) < P and np.all(np.diff(idx) > 0)
    rows = torch.from_numpy(idx.astype(np.int64))
    for k, v in last.items():
        a, b = np.load(tmp_path / "a" / (k + ".npy")), np.load(tmp_path / "b" / (k + ".npy"))
        assert np.array_equal(a, b), f"{k}: a fixed sample"
        want = v if k in ("color", "depth", "uncertainty") else v.index_select(0, rows)
        assert np.array_equal(a, want.float().numpy()), k


def _run(*extra):
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", "small", "--warmup", "1", *extra]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=280)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps_the_last_step(native_lib, tmp_path):
    line = _run("--steps", "3", "--dump-outputs", str(tmp_path / "a"))
    assert all(k in line for k in HEADLINE) and line["steps"] == 3 and line["value"] > 0 and line["ms_per_step"] > 0
    assert abs(line["value"] - 1e3 / line["ms_per_step"]) <= 1e-2 * line["value"]  # (ms_per_step is rounded to 0.1 us)
    assert not {"roofline", "stages", "next_rows", "cpu_baseline", "parity_check", "rotation", "per_rank"} & set(line), "lean by default"
    P, W, H = line["config"]["P"], line["config"]["W"], line["config"]["H"]
    a = {f[:-4]: np.load(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")}
    assert a["color"].shape == (3, H, W) and a["radii"].shape == (P,) and a["grad_means3D"].shape == (P, 3)
    assert all(v.dtype in (np.float32, np.float64) and np.isfinite(v).all() for v in a.values())
    assert (a["radii"] > 0).any() and np.abs(a["grad_colors"]).max() > 0
    # same arguments, same inputs: a second run computes the same outputs (gradients up to the order of their atomic sums)
    _run("--steps", "5", "--dump-outputs", str(tmp_path / "b"))
    b = {f[:-4]: np.load(tmp_path / "b" / f) for f in os.listdir(tmp_path / "b")}
    assert set(a) == set(b) and np.array_equal(a["radii"], b["radii"])
    for k in ("color", "depth", "uncertainty"):
        assert np.allclose(a[k], b[k], rtol=0, atol=1e-5), k
    for k in a:
        if k.startswith("grad_"):
            assert np.linalg.norm(a[k] - b[k]) <= 1e-4 * np.linalg.norm(a[k]), k


@pytest.mark.gpu
def test_full_run_adds_the_extra_objects(native_lib, tmp_path):
    line = _run("--steps", "3", "--full", "--no-cpu-baseline", "--no-next-rows", "--rotation-views", "0", "--dump-outputs", str(tmp_path))
    assert all(k in line for k in HEADLINE) and line["steps"] == 3
    assert {"roofline", "stages", "ms_per_step_spread", "per_rank", "scene_stats", "view_cache"} <= set(line)
    assert os.path.exists(tmp_path / "color.npy")
