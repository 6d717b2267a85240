"""Host cost of NatureConvs.pack()'s early return (it runs several times per minibatch and the per-rank shape is
host-bound: profiles/r06b/R.json, ~601 us of host time per minibatch).

  python tools/pack_hit_cost.py            time the hit path over 100,000 calls, no GPU work (a CPU trunk)
  python tools/pack_hit_cost.py --count    count the pack() calls of one training minibatch (needs the GPU)

Run the first form in two checkouts to compare them: the cost per minibatch is (full-key calls x their time +
in-pass calls x theirs) in each."""
import argparse
import inspect
import json
import os
import sys
import timeit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ppo-exploration_amd")]

import torch  # noqa: E402

import convs  # noqa: E402
import models  # noqa: E402

IN_PASS = "in_pass" in inspect.signature(convs.NatureConvs.pack).parameters


def time_hit(calls=100_000, B=2048):
    torch.manual_seed(0)
    net = models.CnnActorCritic(4, 6)
    flat = models.FlatParams(net, "cpu")
    cv = convs.attach(net, flat, "split")
    real = cv._forms
    cv._forms = lambda batch: set()  # (the first call goes through the miss path: nothing to launch on the CPU)
    cv.pack(B)
    cv._forms = real
    assert cv.pack(B) is False
    out = {"calls": calls, "full_us": min(timeit.repeat(lambda: cv.pack(B), number=calls, repeat=9)) / calls * 1e6}
    if IN_PASS:
        out["in_pass_us"] = min(timeit.repeat(lambda: cv.pack(B, in_pass=True), number=calls, repeat=9)) / calls * 1e6
    return out


def count_calls():
    import ppo
    n = {"full": 0, "in_pass": 0}
    real = convs.NatureConvs.pack

    def counted(self, *a, **k):
        n["in_pass" if k.get("in_pass") else "full"] += 1
        return real(self, *a, **k)
    alg = ppo.PPO(env_id="BreakoutNoFrameskip-v4", n_envs=8, nstep=16, batch_size=32, n_epochs=2, quiet=True)
    alg.collect_samples()
    convs.NatureConvs.pack = counted
    alg.train()
    convs.NatureConvs.pack = real
    torch.cuda.synchronize()
    mbs = int(alg.loss_accum.cpu()[5])
    return {"minibatches": mbs, "full_per_minibatch": n["full"] / mbs, "in_pass_per_minibatch": n["in_pass"] / mbs}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--count", action="store_true")
    args = ap.parse_args()
    print(json.dumps(count_calls() if args.count else time_hit()))
