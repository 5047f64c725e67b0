"""The driver depends on bench.py's CLI and JSON contract; validate it."""

import json
import os
import subprocess
import sys
from pathlib import Path

from dist_utils import launch_env

REPO = Path(__file__).resolve().parent.parent


def _rank_env(n):
    return launch_env(REPO, n)


def test_bench_json_contract():
    env = dict(os.environ)
    env["PYTHONPATH"] = str(REPO)
    env.pop("WORLD_SIZE", None)
    r = subprocess.run(
        [sys.executable, str(REPO / "bench.py"), "--gpus", "1", "--steps", "1",
         "--warmup", "0", "--width", "4", "--num-blocks", "1"],
        capture_output=True, text=True, timeout=900, env=env, cwd=str(REPO))
    assert r.returncode == 0, r.stderr[-2000:]
    line = r.stdout.strip().splitlines()[-1]
    d = json.loads(line)
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup",
                "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                "dtype", "data", "config"):
        assert key in d, f"missing {key}"
    assert d["metric"] == "sec/batch"
    assert d["higher_is_better"] is False
    assert d["scaling"] == "strong"
    assert d["n_gpus"] == 1
    assert d["value"] > 0
    assert abs(d["ms_per_step"] - d["value"] * 1e3) < 1e-6
    assert "synthetic" in d["data"]
    for k in ("model", "global_batch", "parallelism"):
        assert k in d["config"]


def test_bench_dump_outputs_and_full(tmp_path):
    # --dump-outputs writes the last timed step's results as float32 .npy
    # (<= 64 MB in all); --full is accepted and keeps the result line intact
    import numpy as np

    env = dict(os.environ)
    env["PYTHONPATH"] = str(REPO)
    env.pop("WORLD_SIZE", None)
    out = tmp_path / "dump"
    r = subprocess.run(
        [sys.executable, str(REPO / "bench.py"), "--gpus", "1", "--steps", "2",
         "--warmup", "0", "--width", "4", "--num-blocks", "1", "--full",
         "--dump-outputs", str(out)],
        capture_output=True, text=True, timeout=900, env=env, cwd=str(REPO))
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads(r.stdout.strip().splitlines()[-1])
    assert d["metric"] == "sec/batch" and d["steps"] == 2
    assert abs(d["ms_per_step"] - d["value"] * 1e3) < 1e-6
    files = sorted(f.name for f in out.iterdir())
    assert files == ["loss.npy", "params.npy", "y.npy"]
    assert sum(f.stat().st_size for f in out.iterdir()) <= 64 * 2**20
    arrs = {f.stem: np.load(f) for f in out.iterdir()}
    for name, a in arrs.items():
        assert a.dtype == np.float32, name
        assert np.isfinite(a).all(), name
    assert arrs["loss"].shape == (1,) and arrs["loss"][0] > 0
    assert arrs["y"].size == 64 * 64 * 64 * 30
    assert arrs["params"].size > 0 and arrs["params"].std() > 0


def test_bench_json_contract_4rank():
    # the driver launches N>1 exactly like this (torchrun, one rank per GPU);
    # on CPU the world runs over gloo with the same (1,1,2,2,1,1) partition
    env = _rank_env(4)
    r = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
         "--nproc-per-node=4", "--master-addr", "127.0.0.1",
         "--master-port", "29537", str(REPO / "bench.py"), "--gpus", "4",
         "--steps", "1", "--warmup", "0", "--width", "4", "--num-blocks", "1"],
        capture_output=True, text=True, timeout=900, env=env, cwd=str(REPO))
    assert r.returncode == 0, r.stderr[-2000:]
    line = r.stdout.strip().splitlines()[-1]
    d = json.loads(line)
    assert d["n_gpus"] == 4
    assert "2x2" in d["config"]["parallelism"]
    assert d["value"] > 0


def test_bench_json_contract_8rank_driver_partition():
    # the exact launch+partition the driver's 8-GPU SCALE run uses
    env = _rank_env(8)
    r = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
         "--nproc-per-node=8", "--master-addr", "127.0.0.1",
         "--master-port", "29538", str(REPO / "bench.py"), "--gpus", "8",
         "--steps", "1", "--warmup", "0", "--width", "4", "--num-blocks", "1"],
        capture_output=True, text=True, timeout=900, env=env, cwd=str(REPO))
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads(r.stdout.strip().splitlines()[-1])
    assert d["n_gpus"] == 8
    assert "4x2" in d["config"]["parallelism"]
    assert d["value"] > 0


def test_bench_json_contract_8rank_heavy_comm():
    # trailing-axis partition: real R1/R4 all-to-alls + chunk pipeline at 8 ranks
    env = _rank_env(8)
    r = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
         "--nproc-per-node=8", "--master-addr", "127.0.0.1",
         "--master-port", "29539", str(REPO / "bench.py"), "--gpus", "8",
         "--heavy-comm", "--steps", "1", "--warmup", "0", "--width", "4",
         "--num-blocks", "1"],
        capture_output=True, text=True, timeout=900, env=env, cwd=str(REPO))
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads(r.stdout.strip().splitlines()[-1])
    assert d["n_gpus"] == 8
    assert "2x2x2" in d["config"]["parallelism"]
    assert d["value"] > 0
