"""PPO, PPO(sim_hash=True), PPO_RND, PPO_ICM, PPO(episodic=True) and PPO_NGU (defaults, and int_adv_coef=0.3), and the
last two with the elliptical bonus (PPO_E3B, PPO_NGU_E3B), on
KeyDoor-v0 for a fixed number of env steps and three seeds. Every run is a fresh child process under its own `timeout`; its log points (env steps,
ep_rew_mean — the mean return of the last 50 episodes, which on this task is the goal rate —, coverage) go as one
JSON line each into --out, after one line per seed with the numpy twin's random-policy goal rate at that seed and
max_len (tests/keydoor_twin.py, CPU: the reference the learning gate is measured against).  The tool stops at the
first child that exits non-zero.

    python tools/keydoor_compare.py [--steps 655360] [--seeds 11 5 14] [--out profiles/keydoor/compare.jsonl]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
CONFIGS = {
    "PPO": ("PPO", {}),
    "PPO_SimHash": ("PPO", {"sim_hash": True}),
    "PPO_RND": ("PPO_RND", {}),
    "PPO_ICM": ("PPO_ICM", {}),
    "PPO_Episodic": ("PPO", {"episodic": True}),  # the defaults: k 10, capacity max_len, the newest frame
    "PPO_NGU": ("PPO_NGU", {}),                   # the same episodic defaults, mod_max 5, int_adv_coef 1
    "PPO_NGU_0.3": ("PPO_NGU", {"int_adv_coef": 0.3}),
    # the elliptical bonus at its defaults: ridge 2^30, beta 0.1 / mod_max 5, the newest frame
    "PPO_E3B": ("PPO", {"episodic": True, "episodic_kwargs": {"kind": "elliptical"}}),
    "PPO_NGU_E3B": ("PPO_NGU", {"episodic_kwargs": {"kind": "elliptical"}}),
}


def child(args):
    """One run: learn() with a log point per iteration, each printed as a JSON line."""
    sys.path.insert(0, os.path.join(ROOT, "ppo-exploration_amd"))
    import numpy as np
    import torch

    import logger
    import ppo
    from env import make_env
    cls, kw = CONFIGS[args.child]
    np.random.seed(args.seed)
    torch.manual_seed(args.seed)
    env = make_env("KeyDoor-v0", n_envs=args.n_envs, seed=args.seed, dynamics="real", max_len=args.max_len)
    alg = getattr(ppo, cls)(env_id="KeyDoor-v0", dynamics="real", n_envs=args.n_envs, nstep=args.nstep,
                            batch_size=args.batch_size, n_epochs=args.n_epochs, lr=args.lr, seed=args.seed,
                            quiet=True, env=env, **kw)
    real_dump, t0 = logger.dump, time.time()

    def dump(step=0):
        kv = logger.get_values()
        row = {"config": args.child, "seed": args.seed, "env_steps": int(kv["time/total timesteps"]),
               "ep_rew_mean": kv.get("rollout/ep_rew_mean"), "episodes": kv.get("rollout/num_episodes"),
               "coverage": kv["rollout/coverage"], "seconds": round(time.time() - t0, 2)}
        if "rollout/episodic_bonus" in kv:
            row.update(episodic_bonus=kv["rollout/episodic_bonus"])
        if "rollout/episodic_dm" in kv:                    # kind="knn" alone
            row.update(episodic_dm=kv["rollout/episodic_dm"])
        if "rollout/ngu_modulator" in kv:
            row.update(ngu_modulator=kv["rollout/ngu_modulator"], mean_int_reward=kv["rollout/mean_int_reward"])
        print(json.dumps(row), flush=True)
        real_dump(step)

    logger.dump = dump
    alg.learn(total_timesteps=args.steps, log_interval=args.log_interval)
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", choices=list(CONFIGS))
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--seeds", type=int, nargs="+", default=[11, 5, 14])
    ap.add_argument("--configs", nargs="+", default=list(CONFIGS), choices=list(CONFIGS))
    ap.add_argument("--steps", type=int, default=655360)
    ap.add_argument("--max-len", type=int, default=200)
    ap.add_argument("--n-envs", type=int, default=128)
    ap.add_argument("--nstep", type=int, default=128)
    ap.add_argument("--batch-size", type=int, default=2048)
    ap.add_argument("--n-epochs", type=int, default=4)
    ap.add_argument("--lr", type=float, default=5e-4)
    ap.add_argument("--log-interval", type=int, default=1, help="iterations between log points")
    ap.add_argument("--timeout", type=int, default=120, help="seconds per child")
    ap.add_argument("--out", default=os.path.join("profiles", "keydoor", "compare.jsonl"))
    args = ap.parse_args()
    if args.child:
        return child(args)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, ROOT)
    import keydoor_twin as K
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    shared = ["--steps", args.steps, "--max-len", args.max_len, "--n-envs", args.n_envs, "--nstep", args.nstep,
              "--batch-size", args.batch_size, "--n-epochs", args.n_epochs, "--lr", args.lr, "--log-interval", args.log_interval]
    with open(args.out, "w") as out:
        def emit(line):
            out.write(line.rstrip("\n") + "\n")
            out.flush()

        emit(json.dumps({"hyper_parameters": {k: v for k, v in vars(args).items()
                                              if k not in ("child", "seed", "out", "timeout")}}))
        for seed in args.seeds:
            rate, episodes = K.random_policy_rate(seed, max_len=args.max_len)
            emit(json.dumps({"config": "twin_random_policy", "seed": seed, "goal_rate": round(rate, 4),
                             "episodes": episodes, "layout": K.layout(seed)}))
        for config in args.configs:
            for seed in args.seeds:
                cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__),
                       "--child", config, "--seed", str(seed)] + [str(x) for x in shared]
                t0 = time.time()
                proc = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
                lines = [ln for ln in proc.stdout.splitlines() if ln.startswith("{")]
                for ln in lines:
                    emit(ln)
                last = json.loads(lines[-1]) if lines else {}
                print(f"{config} seed {seed}: exit {proc.returncode}, {time.time() - t0:.1f} s, final "
                      f"ep_rew_mean {last.get('ep_rew_mean')}, coverage {last.get('coverage')}", flush=True)
                if proc.returncode != 0:
                    print("stopping: a run exited non-zero", flush=True)
                    return proc.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
