"""Kernel time of ppox_es_evaluate_control (DESIGN.md §8 "ES on the real-dynamics tasks") beside
ppox_es_evaluate at the same population, layer sizes and episode length: P = 10,000 members, hidden (64, 64),
T = the task's max_len, a policy that does not terminate early.  HIP events around each launch, warm, the
median of 21 launches.  Prints one JSON line per figure; --out appends them to a file.

The policies that stay inside the time limit (hidden unit 0 alone carries them, the other weights are 0):
CartPole pushes towards the pole's fall, logits -+200 atan(atan(3 x + 6 x' + 60 theta + 12 theta')); MountainCar
and Acrobot take the idle action (no push / zero torque) off the sign of the position / of cos(theta1), so the
car rocks in the valley and the arm hangs; Pendulum never terminates and runs small random weights.  The step
counts of the population are reported with every figure."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "ppo-exploration_amd"))
import native  # noqa: E402
from env import CONTROL_ENVS  # noqa: E402

P, H = 10000, 64
N_ACT = {"CartPole-v1": 2, "MountainCar-v0": 3, "Acrobot-v1": 3, "Pendulum-v1": 1}


def median_ms(fn, warm=3, iters=21):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        times.append(s.elapsed_time(e))
    return float(np.median(times)), float(min(times)), float(max(times))


def weights(env_id, D, A):
    """[W0, W1, W2] of a policy that stays inside the time limit"""
    if env_id == "Pendulum-v1":
        rs = np.random.RandomState(0)
        return [rs.randn(D, H) / 8, rs.randn(H, H) / 8, rs.randn(H, A) / 8]
    w = [np.zeros((D, H)), np.zeros((H, H)), np.zeros((H, A))]
    w[1][0, 0] = 1.0
    if env_id == "CartPole-v1":
        w[0][:, 0] = (3.0, 6.0, 60.0, 12.0)
        w[2][0] = (-200.0, 200.0)
    elif env_id == "MountainCar-v0":
        w[0][0, 0] = 1.0  # the position is negative in the valley
        w[2][0] = (200.0, -200.0, 200.0)
    else:
        w[0][0, 0] = 1.0  # cos(theta1) is positive while the arm hangs
        w[2][0] = (-200.0, 200.0, -200.0)
    return w


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--population", type=int, default=P)
    args = ap.parse_args()
    n_members = args.population
    rows = []
    for env_id in N_ACT:
        kind, _, D, _, T = CONTROL_ENVS[env_id]
        A = N_ACT[env_id]
        w = torch.from_numpy(np.concatenate([x.reshape(-1) for x in weights(env_id, D, A)])).cuda()
        # eps given, sigma = 0: the population form of the launch (every member reads its own eps row)
        eps = torch.randn(n_members, w.numel(), dtype=torch.float64, device="cuda")
        fit = torch.empty(n_members, dtype=torch.float64, device="cuda")
        steps = torch.empty(n_members, dtype=torch.int32, device="cuda")
        bc = torch.empty(n_members, 2, dtype=torch.float64, device="cuda")

        def real():
            native.es_evaluate_control(kind, w, eps, 0.0, n_members, 0, H, H, T, 12345, 0, fit, steps, bc)
        med, lo, hi = median_ms(real)
        st = steps.cpu().numpy()
        rows.append(dict(kernel="ppox_es_evaluate_control", env=env_id, P=n_members, H1=H, H2=H, T=T, ms=round(med, 3),
                         ms_min=round(lo, 3), ms_max=round(hi, 3), steps_min=int(st.min()),
                         steps_mean=round(float(st.mean()), 1), steps_max=int(st.max()),
                         us_per_step=round(med * 1e3 / max(int(st.max()), 1), 3),
                         env_steps_per_s=round(float(st.sum()) / (med * 1e-3), 0)))
        print(json.dumps(rows[-1]), flush=True)
        # the synthetic kernel at the same P / sizes / T (its own noise table and eps rows)
        xi = torch.empty(T * D, dtype=torch.float64, device="cuda")
        native.es_env_noise(T, D, 12345, xi)
        ws = torch.randn(D * H + H * H + H * A, dtype=torch.float64, device="cuda") / 8
        es = torch.randn(n_members, ws.numel(), dtype=torch.float64, device="cuda")

        def synth():
            native.es_evaluate(ws, es, 0.1, n_members, D, H, H, A, T, 12345, xi, fit, bc)
        med, lo, hi = median_ms(synth)
        rows.append(dict(kernel="ppox_es_evaluate", env=f"synthetic D={D} A={A}", P=n_members, H1=H, H2=H, T=T,
                         ms=round(med, 3), ms_min=round(lo, 3), ms_max=round(hi, 3),
                         us_per_step=round(med * 1e3 / T, 3), env_steps_per_s=round(n_members * T / (med * 1e-3), 0)))
        print(json.dumps(rows[-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
