"""Cost of the episodic novelty bonus on KeyDoor-v0, timed by HIP events.

1. The step's three launches (ppox_simhash_sums_u8 -> ppox_episodic_knn -> ppox_episodic_reward) at --n-envs envs,
   each alone and the three together, single launches after warm-up: once early in the episode (8 embeddings in every
   memory) and once with full memories (count = capacity), for both `frames` settings; beside them the pixel-hash keys
   (ppox_simhash_keys_u8 on the whole stack) and one env step on the same frames, the yardsticks of §4.3 / §11.
   Beside ppox_episodic_reward, on the same kNN outputs: ppox_ngu_reward (PPO_NGU) with the lifelong
   error and without it (RND's warm-up).
2. One learn() iteration (collect_samples + train at --n-envs x --nstep, --batch-size, --n-epochs) of PPO(episodic=True)
   against the default PPO, each in this process after --warmup iterations (the first collect is eager and captures
   the graph), host wall time around a device synchronize.

    python tools/episodic_bench.py [--out profiles/episodic/step_time.json] [--no-iterations]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "ppo-exploration_amd"))
import buffer  # noqa: E402
import env as E  # noqa: E402
import native  # noqa: E402
import ppo  # noqa: E402


def timed(fn, launches, warmup, before=None):
    """Median / min / max microseconds of single calls of fn(), each between two HIP events (before(): run ahead
    of every call, outside the timed window)."""
    out = []
    for i in range(warmup + launches):
        if before is not None:
            before()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if i >= warmup:
            out.append(a.elapsed_time(b) * 1e3)
    return {"median_us": round(statistics.median(out), 2), "min_us": round(min(out), 2), "max_us": round(max(out), 2)}


def step_times(args):
    n, d = args.n_envs, "cuda"
    env = E.DeviceKeyDoorEnv(n_envs=n, seed=0, max_len=args.capacity)
    obs = [torch.empty((n, 4, 84, 84), dtype=torch.uint8, device=d) for _ in range(2)]
    env.reset_into(obs[0])
    actions = torch.randint(0, 5, (n,), dtype=torch.int32, device=d)
    rewards, dones = torch.zeros(n, device=d), torch.zeros(n, dtype=torch.uint8, device=d)
    never = torch.zeros(n, dtype=torch.uint8, device=d)
    dret, dlen = torch.empty(n, device=d), torch.empty(n, dtype=torch.int32, device=d)
    res = {}
    # ppox_ngu_reward's own arguments: lognormal errors, the running moments, the three outputs
    err = torch.randn(n, device=d).mul_(2.0).exp_()
    em = torch.tensor([0.0, 1.0, 1e-4], dtype=torch.float64, device=d)
    ngu_out = torch.zeros((3, n), device=d)
    for frames in ("last", "stack"):
        st = buffer.RolloutStorage(1, n, env.observation_space, env.action_space,
                                   episodic=dict(capacity=args.capacity, frames=frames))
        x = obs[0].reshape(n, -1)[:, st.epi_offset:]
        K, L = st.epi_k, st.epi_capacity
        sums = lambda: native.simhash_sums_u8(x, n, st.epi_D, x.stride(0), st.epi_A8, st.epi_rowsum,  # noqa: E731
                                              st.epi_workspace, st.epi_emb)
        knn = lambda: native.episodic_knn(st.epi_emb, never, n, L, K, st.mem, st.count, st.epi_dk,  # noqa: E731
                                          st.epi_kfound, st.epi_mk)
        rew = lambda: native.episodic_reward(st.epi_dk, st.epi_kfound, st.epi_mk, n, K, st.dm, *st.epi_coef,  # noqa: E731
                                             rewards, st.episodic_bonus[0])
        decay, _, eps, xi, c, smax = st.epi_coef
        ngu = lambda e: native.ngu_reward(st.epi_dk, st.epi_kfound, st.epi_mk, e, n, K, st.dm, em, decay,  # noqa: E731
                                          eps, xi, c, smax, 5.0, ngu_out[0], ngu_out[1], ngu_out[2])
        # memories of random-walk embeddings: 8 rows, then all of them (the timed knn launches keep appending, so
        # the count is put back before each phase; a full ring stays full)
        for j in range(L):
            env.step_into(obs[j % 2], obs[1 - j % 2], actions.random_(0, 5), rewards, dones, dret, dlen)
            st.episodic(obs[1 - j % 2], rewards, never, 0)
        for phase, count in (("early_8_rows", 8), ("full_memory", L)):
            def put_back():
                st.count.fill_(count)
            put_back()
            res[f"{frames}/{phase}"] = {
                "sums": timed(sums, args.launches, args.warmup),
                "knn": timed(knn, args.launches, args.warmup, before=put_back),
                "reward": timed(rew, args.launches, args.warmup),
                "ngu_reward": timed(lambda: ngu(err), args.launches, args.warmup),
                "ngu_reward_no_err": timed(lambda: ngu(None), args.launches, args.warmup),
                "three_launches": timed(lambda: st.episodic(obs[0], rewards, never, 0), args.launches, args.warmup,
                                        before=put_back)}
        del st
        if args.kind == "elliptical":
            res.update(elliptical_step_times(args, env, obs, frames, err, em, ngu_out))
    # the yardsticks, on the same frames
    hs = buffer.RolloutStorage(1, n, env.observation_space, env.action_space, sim_hash=True)
    xs = obs[0].reshape(n, -1)
    res["yardstick/simhash_keys_u8_stack"] = timed(
        lambda: native.simhash_keys_u8(xs, n, xs.shape[1], xs.stride(0), hs.hash_A8, hs.hash_rowsum, hs.hash_workspace,
                                       hs.hash_keys[0]), args.launches, args.warmup)
    res["yardstick/keydoor_env_step"] = timed(
        lambda: env.step_into(obs[0], obs[1], actions, rewards, dones, dret, dlen), args.launches, args.warmup)
    return res


def elliptical_step_times(args, env, obs, frames, err, em, ngu_out):
    """kind="elliptical"  in the same process on the same frames: sums, ppox_elliptical_bonus (with
    the reward add, and bare as PPO_NGU launches it), ppox_ngu_modulate and the two launches together, 8 steps into
    the episode and --capacity steps into it (the matrices dense).  The bonus kernel moves 2 x 2 KB per env."""
    n = args.n_envs
    st = buffer.RolloutStorage(1, n, env.observation_space, env.action_space,
                               episodic=dict(kind="elliptical", frames=frames))
    x = obs[0].reshape(n, -1)[:, st.epi_offset:]
    actions = torch.zeros(n, dtype=torch.int32, device="cuda")
    rewards, dones = torch.zeros(n, device="cuda"), torch.zeros(n, dtype=torch.uint8, device="cuda")
    never = torch.zeros(n, dtype=torch.uint8, device="cuda")
    dret, dlen = torch.empty(n, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda")
    sums = lambda: native.simhash_sums_u8(x, n, st.epi_D, x.stride(0), st.epi_A8, st.epi_rowsum,  # noqa: E731
                                          st.epi_workspace, st.epi_emb)
    ell = lambda: native.elliptical_bonus(st.epi_emb, never, n, st.epi_ridge, st.epi_beta, st.minv,  # noqa: E731
                                          st.count, st.eb, rewards, st.episodic_bonus[0])
    bare = lambda: native.elliptical_bonus(st.epi_emb, never, n, st.epi_ridge, 0.0, st.minv, st.count,  # noqa: E731
                                           st.eb)
    mod = lambda e: native.ngu_modulate(st.eb, e, n, em, 5.0, ngu_out[0], ngu_out[1], ngu_out[2])  # noqa: E731
    res, moved, done_steps = {}, 2 * n * 16 * 16 * 8, 0
    for phase, upto in (("early_8_steps", 8), ("late", args.capacity)):
        for j in range(done_steps, upto):
            env.step_into(obs[j % 2], obs[1 - j % 2], actions.random_(0, 5), rewards, dones, dret, dlen)
            st.episodic(obs[1 - j % 2], rewards, never, 0)
        done_steps = upto
        r = {"sums": timed(sums, args.launches, args.warmup),
             "elliptical_bonus": timed(ell, args.launches, args.warmup),
             "elliptical_bonus_bare": timed(bare, args.launches, args.warmup),
             "ngu_modulate": timed(lambda: mod(err), args.launches, args.warmup),
             "ngu_modulate_no_err": timed(lambda: mod(None), args.launches, args.warmup),
             "two_launches": timed(lambda: st.episodic(obs[0], rewards, never, 0), args.launches, args.warmup)}
        r["elliptical_bonus_GBps_at_median"] = round(moved / r["elliptical_bonus"]["median_us"] * 1e-3, 1)
        res[f"elliptical/{frames}/{phase}"] = r
    res[f"elliptical/{frames}/state_finite"] = bool(torch.isfinite(st.minv).all().item())
    return res


def iteration_times(args):
    res = {}
    configs = [("PPO", {}), ("PPO_episodic", dict(episodic=True))]
    if args.kind == "elliptical":
        configs.append(("PPO_elliptical", dict(episodic=True, episodic_kwargs=dict(kind="elliptical"))))
    for name, kw in configs:
        np.random.seed(0)
        torch.manual_seed(0)
        env = E.make_env("KeyDoor-v0", n_envs=args.n_envs, seed=0, dynamics="real", max_len=args.capacity)
        alg = ppo.PPO(env_id="KeyDoor-v0", dynamics="real", n_envs=args.n_envs, nstep=args.nstep,
                      batch_size=args.batch_size, n_epochs=args.n_epochs, quiet=True, seed=0, env=env, **kw)
        rows = []
        for i in range(args.iter_warmup + args.iterations):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            alg.collect_samples()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            alg.train()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            if i >= args.iter_warmup:
                rows.append((t1 - t0, t2 - t1))
        c, t = statistics.median(r[0] for r in rows), statistics.median(r[1] for r in rows)
        res[name] = {"collect_ms": round(c * 1e3, 2), "train_ms": round(t * 1e3, 2),
                     "iteration_ms": round((c + t) * 1e3, 2), "graphed_collect": alg._cgraph is not None,
                     "env_steps_per_s": round(args.n_envs * args.nstep / (c + t))}
        del alg, env
        torch.cuda.empty_cache()
    res["episodic_over_plain_iteration"] = round(res["PPO_episodic"]["iteration_ms"] / res["PPO"]["iteration_ms"], 4)
    res["collect_added_us_per_step"] = round((res["PPO_episodic"]["collect_ms"] - res["PPO"]["collect_ms"])
                                             / args.nstep * 1e3, 2)
    if args.kind == "elliptical":
        res["elliptical_over_plain_iteration"] = round(res["PPO_elliptical"]["iteration_ms"]
                                                       / res["PPO"]["iteration_ms"], 4)
        res["elliptical_collect_added_us_per_step"] = round(
            (res["PPO_elliptical"]["collect_ms"] - res["PPO"]["collect_ms"]) / args.nstep * 1e3, 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-envs", type=int, default=4096)
    ap.add_argument("--capacity", type=int, default=200, help="ring rows per env = the env's max_len")
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--nstep", type=int, default=128)
    ap.add_argument("--batch-size", type=int, default=16384)
    ap.add_argument("--n-epochs", type=int, default=4)
    ap.add_argument("--iterations", type=int, default=3)
    ap.add_argument("--iter-warmup", type=int, default=2)
    ap.add_argument("--no-iterations", action="store_true", help="the step's launches only")
    ap.add_argument("--kind", choices=("knn", "elliptical"), default="knn",
                    help="elliptical: the kind='elliptical' launches and learn() iteration beside the kNN ones")
    ap.add_argument("--out", default=os.path.join("profiles", "episodic", "step_time.json"))
    args = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0), "config": {k: v for k, v in vars(args).items() if k != "out"},
           "step": step_times(args)}
    if not args.no_iterations:
        out["learn_iteration"] = iteration_times(args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
