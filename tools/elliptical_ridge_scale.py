"""The scale `ridge` of the elliptical bonus is measured against: the squared distance between the
embeddings of successive, distinct observations of a random policy, on the CPU twins of the envs (no GPU).

32 envs x 200 uniformly random steps of KeyDoor-v0 (env seed 11) and Catch-v0 (env seed 3), hash-matrix seed 0, both
`frames` settings; pairs across an episode's end are left out.  Prints one JSON line per (env, frames).

    python tools/elliptical_ridge_scale.py
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import episodic_twin as E  # noqa: E402
import keydoor_twin as K  # noqa: E402
import real_env_twin as R  # noqa: E402
import simhash_px_twin as H  # noqa: E402

N, STEPS, MATRIX_SEED = 32, 200, 0


def measure(name, env, n_actions, frames):
    D = 84 * 84 * (1 if frames == "last" else 4)
    A = H.matrix(D, MATRIX_SEED)
    rs = np.random.RandomState(0)
    prev = E.embed_frames(env.reset(), A, frames).astype(np.int64)
    d2, norms = [], [np.square(prev).sum(axis=1)]
    for _ in range(STEPS):
        out = env.step(rs.randint(0, n_actions, N).astype(np.int32))
        emb = E.embed_frames(out["obs"], A, frames).astype(np.int64)
        d = np.square(emb - prev).sum(axis=1)
        d2.extend(d[(d > 0) & ~out["done"]].tolist())
        norms.append(np.square(emb).sum(axis=1))
        prev = emb
    d2, norms = np.array(d2, np.float64), np.concatenate(norms).astype(np.float64)
    return dict(env=name, frames=frames, pairs=len(d2), d2_median=float(np.median(d2)), d2_min=float(d2.min()),
                d2_max=float(d2.max()), norm2_median=float(np.median(norms)))


def main():
    for frames in ("last", "stack"):
        print(json.dumps(measure("KeyDoor-v0", K.KeyDoorTwin(N, seed=11), 5, frames)))
        print(json.dumps(measure("Catch-v0", R.CatchTwin(N, seed=3), 3, frames)))


if __name__ == "__main__":
    main()
