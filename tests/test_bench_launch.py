"""bench.py's multi-rank launcher: `python bench.py --gpus N` started as a
plain process runs N ranks itself (torch.distributed.run as a child) and rank 0's line carries
n_gpus = N; a rank whose WORLD_SIZE differs from --gpus refuses to report."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _env(**kw):
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(kw)
    return env


def _run(args, env, timeout=240):
    return subprocess.run([sys.executable, BENCH] + args, env=env, capture_output=True, text=True, timeout=timeout)


@pytest.mark.parametrize("n", [2, 3])
def test_gpus_flag_launches_n_ranks(n):
    p = _run(["--gpus", str(n), "--launch-check"], _env(PPOX_DIST_BACKEND="gloo"))
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, p.stdout
    out = json.loads(lines[0])
    assert out["n_gpus"] == n
    assert out["config"]["parallelism"] == f"dp{n}"


def test_world_mismatch_refuses_to_report():
    p = _run(["--gpus", "2", "--launch-check"], _env(WORLD_SIZE="3", RANK="0", LOCAL_RANK="0"))
    assert p.returncode == 2
    assert p.stdout.strip() == ""
    assert "refusing to report" in p.stderr


def test_one_gpu_needs_no_launcher():
    p = _run(["--launch-check"], _env())
    assert p.returncode == 0, p.stderr[-2000:]
    out = json.loads(p.stdout.strip())
    assert out["n_gpus"] == 1 and out["config"]["parallelism"] == "single GPU"


def test_dump_outputs_writes_float_arrays_within_the_budget(tmp_path, monkeypatch):
    """--dump-outputs' writer: every array as <name>.npy in float32 (float64 kept), integer and byte arrays
    converted exactly; an array over its share of the budget is a sample of its elements at fixed sorted
    indices (the same from call to call), so the files together stay within the budget."""
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    rs = np.random.RandomState(3)
    arrays = {"f32": rs.randn(5, 7).astype(np.float32), "f64": rs.randn(9), "i32": np.arange(12, dtype=np.int32),
              "u8": (rs.rand(4, 3) < 0.5).astype(np.uint8), "big": rs.randn(1000).astype(np.float32)}
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 5 * 400)       # 400 B per array: 100 of big's 1000 floats
    bench.dump_outputs(str(tmp_path / "a"), arrays)
    bench.dump_outputs(str(tmp_path / "b"), arrays)
    got = {n: np.load(tmp_path / "a" / (n + ".npy")) for n in arrays}
    assert sorted(os.listdir(tmp_path / "a")) == sorted(n + ".npy" for n in arrays)
    assert {n: g.dtype for n, g in got.items()} == {"f32": np.float32, "f64": np.float64, "i32": np.float32,
                                                    "u8": np.float32, "big": np.float32}
    for n in ("f32", "f64", "i32", "u8"):
        assert got[n].shape == arrays[n].shape and np.array_equal(got[n], arrays[n])
    assert got["big"].shape == (100,)
    idx = np.sort(np.random.RandomState(0).choice(1000, 100, replace=False))
    assert np.array_equal(got["big"], arrays["big"][idx])
    assert np.array_equal(got["big"], np.load(tmp_path / "b" / "big.npy"))
    assert sum(g.nbytes for g in got.values()) <= 5 * 400


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_the_last_steps_outputs(tmp_path):
    """A plain run (no --full) on a tiny config: the line carries the headline fields, value and ms_per_step
    agree, none of --full's legs is there, and --dump-outputs writes the last step's parameters, losses and
    rollout arrays as finite float arrays of the configured shapes."""
    import numpy as np
    d = tmp_path / "out"
    p = _run(["--gpus", "1", "--envs", "64", "--nstep", "16", "--batch-size", "256", "--epochs", "1",
              "--steps", "3", "--warmup", "1", "--dump-outputs", str(d)], _env(), timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    out = json.loads(p.stdout.strip())
    assert out["steps"] == 3 and out["warmup"] == 1 and out["untimed_profiling_iterations"] == 0
    assert out["unit"] == "env-steps/s" and out["higher_is_better"] is True and out["dtype"] == "fp32"
    assert out["ms_per_step"] > 0
    # value and ms_per_step describe the same timed region (each rounded on its own)
    assert out["value"] == pytest.approx(64 * 16 / (out["ms_per_step"] * 1e-3), rel=1e-2)
    for leg in ("roofline", "roofline_solo", "roofline_top", "solo_us", "gae_roofline", "cpu_baseline"):
        assert leg not in out
    got = {f[:-4]: np.load(d / f) for f in os.listdir(d)}
    assert {"policy_params", "loss_accum", "rollout_actions", "rollout_log_probs", "rollout_rewards",
            "rollout_values", "rollout_masks", "rollout_advantages", "rollout_returns"} <= set(got)
    for n, a in got.items():
        assert a.dtype in (np.float32, np.float64), n
        assert np.isfinite(a).all(), n
        if n.startswith("rollout_"):
            assert a.shape == (16, 64), n
    assert got["loss_accum"][5] == 4                     # one epoch of 1024 rows in minibatches of 256
    assert got["policy_params"].size > 1_000_000 and np.abs(got["policy_params"]).max() > 0
    assert sum(a.nbytes for a in got.values()) <= 64 << 20


@pytest.mark.gpu
def test_gpus_2_runs_the_workload_on_two_ranks():
    """The real bench at --gpus 2 on a tiny config, both ranks on the box's one GPU over gloo (RCCL
    refuses two ranks on one device; the driver's N-GPU runs use RCCL, one GPU per rank)."""
    p = _run(["--gpus", "2", "--envs", "64", "--nstep", "16", "--batch-size", "256", "--epochs", "1",
              "--steps", "1", "--warmup", "1", "--no-cpu-baseline"], _env(PPOX_DIST_BACKEND="gloo"), timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    out = json.loads(p.stdout.strip())
    assert out["n_gpus"] == 2 and out["value"] > 0
    assert out["config"]["parallelism"].startswith("dp2")
