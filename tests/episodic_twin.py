"""Numpy twin of the episodic novelty bonus (ppo-exploration_amd/csrc/episodic.hip and
ppox_simhash_sums_u8 of csrc/simhash_px.hip).  The bonus is an extension of this project (the per-episode half
of NGU on integer SimHash projections), so its parity is to this file, written from include/ppox.h:

  emb[n]   = the 16 int sums  sum_d a[b, d] * obs[n, d]  (simhash_px_twin.projections, int64 accumulation)
  d2_j     = sum_i (emb[n, i] - mem[n, j, i])^2 over the env's live ring rows, exact integers
  dk       = the k = min(K, live) smallest d2 ascending, as float64; mk = (dk[0] + dk[1] + ...) / k
  S        = adjacent-pair tree sum of mk over the env index; dm = running mean of S / n_valid
  r        = 1 / (sqrt(sum_i eps / (max(dk_i / dm - xi, 0) + eps)) + c), 0 when the root exceeds smax
  rewards  = f32(rewards + f32(beta * r)), one float32 add
Test infrastructure only.
"""
import numpy as np

import simhash_px_twin as H

EMB = 16
DEFAULTS = {"k": 10, "capacity": 256, "beta": 0.1, "eps": 1e-3, "xi": 8e-3, "c": 1e-3, "smax": 8.0, "decay": 0.99,
            "frames": "last"}


def sums(obs, A8):
    """(n, 16) int32 embeddings of uint8 rows (int64 accumulation; they fit int32 for 16 * 255 * D < 2^31)."""
    p = H.projections(obs, A8)
    assert np.abs(p).max(initial=0) < 2 ** 31
    return p.astype(np.int32)


def sq_dists(e, rows):
    """Exact squared distances of the embedding e (16,) to rows (m, 16) in int64; the bound that keeps them exact
    (|difference| < 2^28) is asserted, so the twin itself cannot overflow silently."""
    diff = rows.astype(np.int64) - np.asarray(e, np.int64)[None, :]
    assert np.abs(diff).max(initial=0) < 2 ** 28
    return (diff * diff).sum(axis=1)  # each square < 2^56, 16 of them < 2^60


def knn(e, rows, K):
    """The k = min(K, m) smallest squared distances, ascending, by a full sort -> (dk (k,) float64, mean)."""
    d = np.sort(sq_dists(e, rows))[:K]
    dk = d.astype(np.float64)          # int64 -> float64 rounds to nearest
    s = 0.0
    for x in dk:                       # added in ascending order
        s = s + x
    return dk, (s / len(dk) if len(dk) else 0.0)


def tree_sum(x):
    """Adjacent pairs, level by level, zero-padded to a power of two."""
    a = np.asarray(x, np.float64)
    p = 1
    while p < len(a):
        p *= 2
    a = np.concatenate([a, np.zeros(p - len(a))])
    while len(a) > 1:
        a = a[0::2] + a[1::2]
    return float(a[0]) if len(a) else 0.0


class Episodic:
    """The device state and one step of it: mem (N, L, 16) int32, count (N,) int32, dm (2,) float64."""

    def __init__(self, N, L, K=10, beta=0.1, eps=1e-3, xi=8e-3, c=1e-3, smax=8.0, decay=0.99):
        self.N, self.L, self.K = N, L, K
        self.beta, self.eps, self.xi, self.c, self.smax, self.decay = beta, eps, xi, c, smax, decay
        self.mem = np.zeros((N, L, EMB), np.int32)
        self.count = np.zeros(N, np.int32)
        self.dm = np.zeros(2, np.float64)
        # which branches the steps so far have taken (the GPU tests assert on these)
        self.seen = {"wrap": 0, "reset": 0, "k_lt_K": 0, "s_gt_smax": 0, "dm_zero": 0}

    def knn_step(self, emb, done):
        """-> dk (N, K) zero-padded, kfound (N,), mk (N,); then the append / reset."""
        N, L, K = self.N, self.L, self.K
        dk, kfound, mk = np.zeros((N, K)), np.zeros(N, np.int32), np.zeros(N)
        for n in range(N):
            m = min(int(self.count[n]), L)
            d, mean = knn(emb[n], self.mem[n, :m], K)
            dk[n, :len(d)], kfound[n], mk[n] = d, len(d), mean
            if 0 < len(d) < K:
                self.seen["k_lt_K"] += 1
            if self.count[n] >= L:
                self.seen["wrap"] += 1
            self.mem[n, int(self.count[n]) % L] = emb[n]
            if done[n]:
                self.count[n] = 0
                self.seen["reset"] += 1
            else:
                self.count[n] += 1
        return dk, kfound, mk

    def reward_step(self, dk, kfound, mk, rewards):
        """-> (rewards' (N,) float32, bonus (N,) float32); dm advanced."""
        valid = kfound > 0
        S = tree_sum(np.where(valid, mk, 0.0))
        if valid.any():
            mu = S / float(valid.sum())
            self.dm[0] = mu if self.dm[1] == 0 else self.decay * self.dm[0] + (1.0 - self.decay) * mu
            self.dm[1] += 1
        d0 = self.dm[0]
        r = np.zeros(self.N)
        for n in np.flatnonzero(valid):
            acc = 0.0
            for i in range(kfound[n]):
                q = dk[n, i] / d0 if d0 > 0 else 0.0
                q = max(q - self.xi, 0.0)
                acc = acc + self.eps / (q + self.eps)
            s = np.sqrt(acc) + self.c
            if s > self.smax:
                self.seen["s_gt_smax"] += 1
            r[n] = 0.0 if s > self.smax else 1.0 / s
            if not d0 > 0:
                self.seen["dm_zero"] += 1
        bonus = r.astype(np.float32)
        add = (self.beta * r).astype(np.float32)
        return np.asarray(rewards, np.float32) + add, bonus

    def step(self, emb, done, rewards):
        dk, kfound, mk = self.knn_step(np.asarray(emb, np.int32), np.asarray(done))
        return self.reward_step(dk, kfound, mk, rewards)


# ------------------------------------------------------------------------------------------------ test cases
# The memory-and-bonus cases both test files drive (the CPU file checks that each case reaches the branches it
# is there for, the GPU file compares the kernels with the twin step by step).  L x K is fully crossed (K > L and
# K > live rows included); N, the done pattern, the embedding kind and smax rotate over that grid so that every
# value meets every L and several K; three more cases pin what the rotation leaves out.
#   kind "small":     coordinates from {-1, 0, 1}, only the first 2 non-zero: duplicates and zero distances common
#        "extreme":   coordinates +-(2^27 - 1): squared distances up to 2^60
#        "identical": one embedding for every env and step: dm[0] stays 0
#   done "never" / "always" / "bern" (Bernoulli(0.1))
#   smax 1.5 puts sqrt(k) + c above it as soon as k >= 3 near-duplicates are found (8, the default, is out of
#   reach for K <= 16: the sum is at most k)
EXTREME = 2 ** 27 - 1
_NS, _DONES = (1, 3, 64, 65, 257), ("never", "always", "bern")


def _grid():
    out = []
    for i, (L, K) in enumerate((L, K) for L in (1, 2, 5, 40) for K in (1, 3, 10, 16)):
        out.append(dict(N=_NS[i % 5], L=L, K=K, kind="extreme" if i % 4 == 3 else "small", done=_DONES[i % 3],
                        smax=1.5 if i % 2 else 8.0, seed=100 + i))
    out.append(dict(N=65, L=5, K=10, kind="identical", done="never", smax=8.0, seed=200))
    out.append(dict(N=3, L=40, K=16, kind="extreme", done="bern", smax=8.0, seed=201))
    out.append(dict(N=257, L=2, K=3, kind="small", done="bern", smax=1.5, seed=202))
    out.append(dict(N=64, L=5, K=3, kind="identical", done="bern", smax=1.5, seed=203))
    return out


CASES = _grid()


def case_id(c):
    return f"N{c['N']}-L{c['L']}-K{c['K']}-{c['kind']}-{c['done']}-smax{c['smax']}"


def case_inputs(c):
    """The case's 3 L + 2 steps: (emb (S, N, 16) int32, done (S, N) uint8, rewards (S, N) float32)."""
    rs = np.random.RandomState(c["seed"])
    S, N = 3 * c["L"] + 2, c["N"]
    if c["kind"] == "small":
        emb = np.zeros((S, N, EMB), np.int32)
        emb[..., :2] = rs.randint(-1, 2, (S, N, 2))
    elif c["kind"] == "extreme":
        emb = (rs.randint(0, 2, (S, N, EMB)) * 2 - 1).astype(np.int32) * EXTREME
    else:
        emb = np.broadcast_to(rs.randint(-1000, 1000, EMB).astype(np.int32), (S, N, EMB)).copy()
    done = {"never": np.zeros((S, N), bool), "always": np.ones((S, N), bool),
            "bern": rs.rand(S, N) < 0.1}[c["done"]].astype(np.uint8)
    return emb, done, rs.randn(S, N).astype(np.float32)


def case_branches(c):
    """The branches the case must reach (keys of Episodic.seen), from its parameters alone."""
    need = set()
    if c["done"] == "never" or (c["done"] == "bern" and c["L"] <= 5):
        need.add("wrap")                      # 3 L + 2 steps against a ring of L
    if c["done"] != "always":
        if c["K"] > 1:
            need.add("k_lt_K")                # the second step of an episode finds one row
    if c["done"] != "never":
        need.add("reset")
    if c["smax"] < 2 and c["K"] >= 3 and c["L"] >= 3 and c["done"] != "always" and c["kind"] != "extreme":
        need.add("s_gt_smax")
    if c["kind"] == "identical":
        need.add("dm_zero")
    return need


def embed_frames(obs, A8, frames):
    """obs (N, C, H, W) uint8 -> (N, 16) int32 of the newest frame ("last") or the whole stack ("stack")."""
    x = obs[:, -1] if frames == "last" else obs
    return sums(x.reshape(x.shape[0], -1), A8)


def replay(state, A8, frames, obs_slots, masks, plain_rewards):
    """A recorded rollout through the twin: obs_slots (T, N, C, H, W) uint8, masks (T, N), plain_rewards (T, N)
    float32 (the env's rewards before the bonus) -> (rewards (T, N) float32, bonus (T, N) float32).  `state`
    (an Episodic) carries over to the next rollout."""
    T, N = masks.shape
    rew, bonus = np.empty((T, N), np.float32), np.empty((T, N), np.float32)
    for t in range(T):
        rew[t], bonus[t] = state.step(embed_frames(obs_slots[t], A8, frames), masks[t], plain_rewards[t])
    return rew, bonus
