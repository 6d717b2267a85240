"""K12 self-imitation timings: the ppox_sil_* kernels by graph replay (as
tools/gae_sweep.py: the host's per-launch cost is not in the figure) and a PPO iteration with
`sil` on against off on the real-dynamics CartPole-v1 and Catch-v0.  Prints one JSON line per figure."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "ppo-exploration_amd"))
import native  # noqa: E402
from gae_sweep import time_ms  # noqa: E402


def emit(**kw):
    print(json.dumps(kw), flush=True)


def ring_tensors(S, N, P):
    d = "cuda"
    return {"obs": None, "actions": torch.zeros((S, N), dtype=torch.int32, device=d),
            "log_probs": torch.zeros((S, N), device=d), "returns": torch.zeros((S, N), device=d),
            "dones": torch.zeros((S, N), dtype=torch.uint8, device=d),
            "state": torch.zeros((S, N), dtype=torch.uint8, device=d),
            "sum_tree": torch.zeros(2 * P, dtype=torch.float64, device=d),
            "min_tree": torch.full((2 * P,), float("inf"), dtype=torch.float64, device=d)}


def kernels():
    d = "cuda"
    # append / returns / rebuild at the benchmark's rollout: 4,096 envs x 128 steps into a ring of 256 steps
    T, N, S = 128, 4096, 256
    P = 1 << (S * N - 1).bit_length()
    ring = ring_tensors(S, N, P)
    acts = torch.randint(0, 4, (T, N), dtype=torch.int32, device=d)
    lps, rews = -torch.rand(T, N, device=d), torch.randn(T, N, device=d)
    dones = (torch.rand(T, N, device=d) < 0.01).to(torch.uint8)
    mp = torch.ones(1, dtype=torch.float64, device=d)
    na = torch.zeros(1, dtype=torch.int64, device=d)
    t_app = time_ms(lambda: native.sil_append(None, acts, lps, rews, dones, ring, 0))

    def app_ret():  # (the returns need freshly pending slots: timed with its append, then the difference)
        native.sil_append(None, acts, lps, rews, dones, ring, 0)
        native.sil_returns(ring, T - 1, 0.99, 0.6, mp)
    t_both = time_ms(app_ret)
    emit(kernel="ppox_sil_append", T=T, N=N, S=S, us=round(t_app * 1e3, 2), note="no observation copy")
    emit(kernel="ppox_sil_returns", T=T, N=N, S=S, us=round((t_both - t_app) * 1e3, 2),
         note="append + returns minus append")
    t_reb = time_ms(lambda: native.sil_tree_rebuild(ring["sum_tree"], ring["min_tree"], ring["state"], na))
    emit(kernel="ppox_sil_tree_rebuild", P=P, slots=S * N, us=round(t_reb * 1e3, 2))

    # one SIL epoch's kernels at B = 128, P = 65,536 (the default buffer at 8 envs)
    B, A, S, N = 128, 4, 8192, 8
    P = 65536
    ring = ring_tensors(S, N, P)
    leaves = torch.rand(P, dtype=torch.float64, device=d) + 1e-3
    ring["sum_tree"][P:], ring["min_tree"][P:] = leaves, leaves
    ring["state"].fill_(2)
    ring["actions"].copy_(torch.randint(0, A, (S, N), device=d))
    ring["returns"].normal_()
    native.sil_tree_rebuild(ring["sum_tree"], ring["min_tree"], ring["state"], na)
    t_reb = time_ms(lambda: native.sil_tree_rebuild(ring["sum_tree"], ring["min_tree"], ring["state"], na))
    emit(kernel="ppox_sil_tree_rebuild", P=P, slots=S * N, us=round(t_reb * 1e3, 2))
    u = torch.rand(B, dtype=torch.float64, device=d)
    idx = torch.empty(B, dtype=torch.int64, device=d)
    w = torch.empty(B, device=d)
    logits, values = torch.randn(B, A, device=d), torch.randn(B, device=d)
    dz, dv, pri = torch.empty(B, A, device=d), torch.empty(B, device=d), torch.empty(B, device=d)
    partials = torch.zeros(native.LOSS_PARTIALS * 4, dtype=torch.float64, device=d)
    accum = torch.zeros(3, dtype=torch.float64, device=d)
    t_s = time_ms(lambda: native.sil_sample(ring["sum_tree"], ring["min_tree"], na, u, 1.0, idx, w))
    t_l = time_ms(lambda: native.sil_loss(logits, values, idx, ring, w, 0.2, 0.01, dz, dv, pri, partials, accum))
    t_u = time_ms(lambda: native.sil_update_priorities(idx, pri, 0.6, ring["sum_tree"], ring["min_tree"], mp))
    for name, t in (("ppox_sil_sample", t_s), ("ppox_sil_loss", t_l), ("ppox_sil_update_priorities", t_u)):
        emit(kernel=name, B=B, P=P, A=A, us=round(t * 1e3, 2))


def iteration_ms(env_id, sil, iters, **kw):
    import logger
    import ppo
    logger.configure("PPO", env_id, quiet=True)
    np.random.seed(0)
    alg = ppo.PPO(env_id=env_id, dynamics="real", sil=sil, quiet=True, **kw)
    for _ in range(3):  # warm-up: the captured collect graph, the library GEMMs, an active ring
        alg.collect_samples()
        alg.train()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        alg.collect_samples()
        alg.train()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3, (len(alg.sil_module.buffer) if sil else 0)


def iterations():
    for env_id, kw, iters in (("CartPole-v1", dict(n_envs=8, nstep=128), 20),
                              ("Catch-v0", dict(n_envs=8, nstep=128, sil_kwargs=dict(size=8192)), 10)):
        for sil in (False, True):
            k = dict(kw)
            if not sil:
                k.pop("sil_kwargs", None)
            ms, active = iteration_ms(env_id, sil, iters, **k)
            emit(iteration=env_id, sil=sil, ms=round(ms, 2), active_slots=active, **{a: b for a, b in k.items()
                                                                                      if a != "sil_kwargs"})


if __name__ == "__main__":
    kernels()
    if "--kernels-only" not in sys.argv:
        iterations()
