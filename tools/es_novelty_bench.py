"""Kernel time of ppox_es_knn_novelty (DESIGN.md §8 "Novelty per member") at the C5 population, P = 10,000 members,
D = 2, K = 10, against archives of M = 1, 100, 1,000 and 10,000 rows — beside the host route it replaces
(EvolutionStrategy.get_kNN called once per member on the same box, timed on --host-members members and scaled to
P) and beside the archive's bytes over the kernel time.  Then one generation of run() with novelty="scalar" and
with novelty="member" at P = 10,000 on CartPole-v1 (wall time per generation, device synchronised, the median
over the generations after the first three).  The method of tools/es_control_bench.py: HIP events around each
launch, 3 warm launches, the median of 21.  Prints one JSON line per figure; --out appends them to a file
(default profiles/es_novelty/knn.jsonl)."""
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
import native  # noqa: E402

P, D, K = 10000, 2, 10
ARCHIVES = (1, 100, 1000, 10000)


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


def kernel_rows(n_members, host_members):
    rs = np.random.RandomState(0)
    bc_h = rs.randn(n_members, D)
    bc = torch.from_numpy(bc_h).cuda()
    out = torch.empty(n_members, dtype=torch.float64, device="cuda")
    for M in ARCHIVES:
        arch_h = rs.randn(M, D)
        arch = torch.from_numpy(arch_h).cuda()
        med, lo, hi = median_ms(lambda: native.es_knn_novelty(bc, arch, K, out))
        # the host route: the class's get_kNN, one member at a time, on the list of (1, 2) rows run() keeps
        rows = [arch_h[m:m + 1] for m in range(M)]
        S = min(K, M)
        n = min(host_members, n_members)
        t0 = time.perf_counter()
        host = [ES.EvolutionStrategy.get_kNN(None, rows, bc_h[p], S) / S for p in range(n)]
        host_ms = (time.perf_counter() - t0) * 1e3 * n_members / n
        got = out[:n].cpu().numpy()
        want = np.where(np.array(host) <= 1e-3, 5e-3, host)
        yield dict(kernel="ppox_es_knn_novelty", P=n_members, D=D, K=K, M=M, ms=round(med, 4), ms_min=round(lo, 4),
                   ms_max=round(hi, 4), archive_bytes=M * D * 8,
                   archive_gb_per_s=round(M * D * 8 / (med * 1e-3) / 1e9, 4),
                   pairs_per_s=round(n_members * M / (med * 1e-3), 0),
                   host_get_knn_ms=round(host_ms, 1), host_members_timed=n,
                   max_rel_diff_from_host=float((np.abs(got - want) / want).max()))


def generation_rows(n_members, generations):
    for mode in ("scalar", "member"):
        np.random.seed(0)
        es = ES.EvolutionStrategy("CartPole-v1", [8, 8], population_size=n_members, sigma=0.1, learning_rate=0.2,
                                  seed=0, dynamics="real", novelty=mode)
        stamps = []
        inner = es._get_population

        def stamped(inner=inner):  # the first call of every generation
            torch.cuda.synchronize()
            stamps.append(time.perf_counter())
            return inner()
        es._get_population = stamped
        es.run(generations, log_interval=10 ** 9)
        per_gen = np.diff(stamps)[3:] * 1e3
        yield dict(figure="run() generation", env="CartPole-v1", P=n_members, hidden=[8, 8], novelty=mode,
                   generations=generations, ms_per_generation=round(float(np.median(per_gen)), 3),
                   ms_min=round(float(per_gen.min()), 3), ms_max=round(float(per_gen.max()), 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "es_novelty", "knn.jsonl"))
    ap.add_argument("--population", type=int, default=P)
    ap.add_argument("--host-members", type=int, default=500)
    ap.add_argument("--generations", type=int, default=16)
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for rows in (kernel_rows(args.population, args.host_members), generation_rows(args.population, args.generations)):
        for row in rows:
            print(json.dumps(row), flush=True)
            with open(args.out, "a") as f:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
