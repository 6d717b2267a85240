"""Timing of the pixel SimHash keys (csrc/simhash_px.hip ppox_simhash_keys_u8: int8 MFMA on the uint8 frames
in place) against the only route to keys of frames without it: obs.float() followed by ppox_simhash_keys on
the f32 rows (f64 matrix), conversion included.  HIP events on the launch stream, warm-up, the two routes
alternated over several rounds (median reported, the spread beside it), one JSON line per N at D = 4*84*84.
GB/s are over the algorithmic bytes N * D (each frame byte read once); the fraction is of 8 TB/s.
--collect adds PPO.collect_samples() at 4096 envs x 128 steps with sim_hash=True against sim_hash=False.
Usage: python tools/simhash_u8_bench.py [--collect] [N ...]"""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ppo-exploration_amd"))
import native  # noqa: E402

D = 4 * 84 * 84
PEAK = 8e12


def window(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps * 1e3  # us


def keys_bench(N, rounds=5):
    g = torch.Generator(device="cuda").manual_seed(N)
    obs = torch.randint(0, 256, (N, D), dtype=torch.uint8, device="cuda", generator=g)
    A8 = torch.empty((16, D), dtype=torch.int8, device="cuda")
    rowsum = torch.empty(16, dtype=torch.int32, device="cuda")
    native.simhash_matrix_i8(D, 0, A8, rowsum)
    ws = torch.empty(native.simhash_keys_u8_workspace_bytes(N) // 4, dtype=torch.int32, device="cuda")
    keys = torch.empty(N, dtype=torch.int32, device="cuda")
    A64 = torch.randn(16, D, dtype=torch.float64, device="cuda", generator=g)
    keys_f = torch.empty(N, dtype=torch.int32, device="cuda")

    def new():
        native.simhash_keys_u8(obs, N, D, D, A8, rowsum, ws, keys)

    def old():
        x = obs.float()
        native.simhash_keys(x, N, D, D, A64, keys_f)

    for _ in range(3):
        new()
    old()
    t_new, t_old = [], []
    for _ in range(rounds):  # 1000 / 20 timed calls in all (the float route walks 28,224 strided floats per thread)
        t_new.append(window(new, 200))
        t_old.append(window(old, 4))
    # the unchanged second half of the bonus (ppox_simhash_apply: rank among same-key envs + table update) on these keys
    table = torch.zeros(native.SIMHASH_KEYS, dtype=torch.int32, device="cuda")
    rew = torch.zeros(N, device="cuda")
    apply_us = statistics.median(
        window(lambda: native.simhash_apply(keys, N, 0, N, table, 0.1, rew), 200) for _ in range(rounds))
    n, o = statistics.median(t_new), statistics.median(t_old)
    gbs = lambda us: N * D / (us * 1e-6) / 1e9  # noqa: E731
    return {"N": N, "D": D, "u8_mfma_us": round(n, 2), "u8_mfma_us_min_max": [round(min(t_new), 2), round(max(t_new), 2)],
            "u8_mfma_GBps": round(gbs(n), 1), "u8_mfma_frac_of_8TBps": round(gbs(n) * 1e9 / PEAK, 4),
            "float_f64_route_us": round(o, 1), "float_f64_route_us_min_max": [round(min(t_old), 1), round(max(t_old), 1)],
            "float_f64_route_GBps": round(gbs(o), 2), "float_f64_route_frac_of_8TBps": round(gbs(o) * 1e9 / PEAK, 5),
            "speedup": round(o / n, 1), "apply_us": round(apply_us, 2)}


def collect_bench(n_envs=4096, nstep=128, timed=3):
    import logger
    import ppo
    logger.configure("PPO", "BreakoutNoFrameskip-v4", quiet=True)
    out = {"n_envs": n_envs, "nstep": nstep, "env_id": "BreakoutNoFrameskip-v4"}
    for flag in (False, True):
        np.random.seed(0)
        torch.manual_seed(0)
        alg = ppo.PPO(env_id="BreakoutNoFrameskip-v4", n_envs=n_envs, nstep=nstep, batch_size=16384, n_epochs=1,
                      quiet=True, seed=0, sim_hash=flag)
        for _ in range(2):  # the eager first collect + capture, then one replay
            alg.collect_samples()
        ts = []
        for _ in range(timed):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            alg.collect_samples()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        out["collect_ms_sim_hash_%s" % flag] = round(statistics.median(ts), 2)
        out["collect_ms_sim_hash_%s_all" % flag] = [round(t, 2) for t in ts]
        out["graphed_sim_hash_%s" % flag] = alg._cgraph is not None
        del alg
        torch.cuda.empty_cache()
    out["overhead_ms"] = round(out["collect_ms_sim_hash_True"] - out["collect_ms_sim_hash_False"], 2)
    out["overhead_us_per_step"] = round(out["overhead_ms"] * 1e3 / nstep, 1)
    return out


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--collect"]
    for N in [int(x) for x in args] or [512, 4096]:
        print(json.dumps(keys_bench(N)), flush=True)
    if "--collect" in sys.argv[1:]:
        print(json.dumps(collect_bench()), flush=True)
