"""Does ES learn on the real-dynamics control tasks, and does the novelty term help (DESIGN.md §8 "ES on the
real-dynamics tasks")?  Seeds 0, 1, 2 on CartPole-v1 and MountainCar-v0, each run twice: ES-NSRA as shipped
(EvolutionStrategy.run) and plain ES (the same population, evaluation and update with the novelty term off:
_update_weights(rewards, population, None)).  Per generation it records the population's mean fitness and mean
episode length and the share of members that reached the goal (CartPole: the full time limit; MountainCar: the
flag, i.e. an episode shorter than the limit), with the wall time since the start of the run.  One JSON line per
run, appended to --out (default profiles/es_control/compare.jsonl).

--modes also takes `member`: EvolutionStrategy(..., novelty="member").run, the novelty of every member against the
archive in the update (DESIGN.md §8 "Novelty per member"); with it the default --out is
profiles/es_novelty/compare.jsonl.  Every row carries first_goal_gen, the first generation in which any member
reached the goal (null: none did)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "ppo-exploration_amd"))
import evolution_strategies as ES  # noqa: E402
import logger  # noqa: E402


def make(env_id, seed, args, mode="nsra"):
    np.random.seed(seed)
    kw = dict(novelty="member") if mode == "member" else {}
    es = ES.EvolutionStrategy(env_id, list(args.hidden), population_size=args.population, sigma=args.sigma,
                              learning_rate=args.lr, seed=seed, dynamics="real", **kw)
    hist = dict(fitness=[], ep_len=[], goal=[], t=[])
    inner = es._get_rewards
    t0 = [None]

    def record(rewards):
        steps = es.ep_len
        goal = steps == es.T if env_id.startswith("CartPole") else steps < es.T
        hist["fitness"].append(float(rewards.mean()))
        hist["ep_len"].append(float(steps.mean()))
        hist["goal"].append(float(goal.mean()))
        hist["t"].append(time.perf_counter() - t0[0])

    def recorded(pool, population):
        rewards = inner(pool, population)
        record(rewards)
        return rewards
    es._get_rewards = recorded
    if mode == "member":  # run() evaluates through the launch that also asks for the behaviours
        inner_member = es._get_rewards_novelty

        def recorded_member(population):
            rewards, novelty = inner_member(population)
            record(rewards)
            return rewards, novelty
        es._get_rewards_novelty = recorded_member
    return es, hist, t0


def run_one(env_id, seed, mode, args):
    es, hist, t0 = make(env_id, seed, args, mode)
    torch.cuda.synchronize()
    t0[0] = time.perf_counter()
    if mode in ("nsra", "member"):
        es.run(args.generations, log_interval=10 ** 9)
    else:
        logger.configure("ES", env_id, quiet=True)
        for g in range(args.generations):
            es.generation = g
            population = es._get_population()
            es._update_weights(es._get_rewards(None, population), population, None)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0[0]
    f = hist["fitness"]
    hit = np.flatnonzero(np.array(hist["goal"]) > 0)
    return dict(first_goal_gen=int(hit[0]) if len(hit) else None,
                t_first_goal=round(hist["t"][int(hit[0])], 3) if len(hit) else None,env=env_id, seed=seed, mode=mode, population=args.population, hidden=list(args.hidden),
                sigma=args.sigma, lr=args.lr, generations=args.generations, wall_s=round(wall, 3),
                fitness_gen0=round(f[0], 3), fitness_last5=round(float(np.mean(f[-5:])), 3),
                ep_len_gen0=round(hist["ep_len"][0], 2), ep_len_last5=round(float(np.mean(hist["ep_len"][-5:])), 2),
                goal_rate_last5=round(float(np.mean(hist["goal"][-5:])), 4),
                goal_rate_any=round(float(np.mean(np.array(hist["goal"]) > 0)), 4),
                novelty_param_end=float(es.novelty_param),
                fitness=[round(x, 2) for x in f], ep_len=[round(x, 2) for x in hist["ep_len"]],
                goal=[round(x, 4) for x in hist["goal"]], t=[round(x, 3) for x in hist["t"]])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", nargs="+", default=["CartPole-v1", "MountainCar-v0"])
    ap.add_argument("--seeds", nargs="+", type=int, default=[0, 1, 2])
    ap.add_argument("--generations", type=int, default=100)
    ap.add_argument("--population", type=int, default=64)
    ap.add_argument("--hidden", nargs=2, type=int, default=[8, 8])
    ap.add_argument("--sigma", type=float, default=0.1)
    ap.add_argument("--lr", type=float, default=0.2)
    ap.add_argument("--modes", nargs="+", default=["nsra", "plain"], choices=["nsra", "plain", "member"])
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "es_novelty" if "member" in args.modes else "es_control",
                                "compare.jsonl")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for env_id in args.envs:
        for seed in args.seeds:
            for mode in args.modes:
                row = run_one(env_id, seed, mode, args)
                with open(args.out, "a") as f:
                    f.write(json.dumps(row) + "\n")
                print(json.dumps({k: v for k, v in row.items() if k not in ("fitness", "ep_len", "goal", "t")}),
                      flush=True)


if __name__ == "__main__":
    main()
