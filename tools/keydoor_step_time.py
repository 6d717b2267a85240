"""One KeyDoor-v0 step against one Catch-v0 step at the same env count: both move the same
frame bytes (N x 28,224 B read and written), so a difference is the render (144 cell values built in LDS and
16 byte reads of them per chunk, against Catch's compare-and-select per pixel) and the visit count.  Single
launches timed by HIP events after warm-up, the two envs alternating; medians into --out."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "ppo-exploration_amd"))
import env as E  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-envs", type=int, default=4096)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join("profiles", "keydoor", "step_time.json"))
    args = ap.parse_args()
    n, d = args.n_envs, "cuda"
    runs = {}
    for name, env, n_actions in (("Catch-v0", E.DeviceCatchEnv(n_envs=n, seed=0), 3),
                                 ("KeyDoor-v0", E.DeviceKeyDoorEnv(n_envs=n, seed=0), 5)):
        obs = [torch.empty((n, 4, 84, 84), dtype=torch.uint8, device=d) for _ in range(2)]
        env.reset_into(obs[0])
        runs[name] = dict(env=env, obs=obs, times=[],
                          actions=torch.randint(0, n_actions, (n,), dtype=torch.int32, device=d),
                          rewards=torch.empty(n, device=d), dones=torch.empty(n, dtype=torch.uint8, device=d),
                          done_ret=torch.empty(n, device=d), done_len=torch.empty(n, dtype=torch.int32, device=d))
    for i in range(args.warmup + args.launches):
        for r in runs.values():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            r["env"].step_into(r["obs"][i % 2], r["obs"][1 - i % 2], r["actions"], r["rewards"], r["dones"],
                               r["done_ret"], r["done_len"])
            b.record()
            b.synchronize()
            if i >= args.warmup:
                r["times"].append(a.elapsed_time(b) * 1e3)
    frame_bytes = 2 * n * 4 * 84 * 84
    out = {"n_envs": n, "launches": args.launches, "warmup": args.warmup, "bytes_read_and_written": frame_bytes,
           "device": torch.cuda.get_device_name(0)}
    for name, r in runs.items():
        med = statistics.median(r["times"])
        out[name] = {"median_us": round(med, 2), "min_us": round(min(r["times"]), 2),
                     "max_us": round(max(r["times"]), 2), "GB_per_s_at_median": round(frame_bytes / med / 1e3, 1)}
    out["keydoor_over_catch"] = round(out["KeyDoor-v0"]["median_us"] / out["Catch-v0"]["median_us"], 3)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
