"""Numpy twin of the pixel SimHash (ppo-exploration_amd/csrc/simhash_px.hip).

The reference has no usable image hash (it draws A = randn(16, obs_shape[0]) and keys on the
string of a summarised array), so the pixel count bonus is an extension of this project and its
parity is to this file, written from the definition:
  a[b, d] = popcount(w & 0xFFFF) - popcount(w >> 16), w = word d % 4 of
            philox4x32_10({d / 4, b, 0, 0xFFFFFFFE}, key = (seed lo32, seed hi32))
  key     = sum_b 2^b [ sum_d a[b, d] * obs[d] > 0 ],  obs the flattened bytes as unsigned 0..255
  bonus   = the sequential dictionary update of buffer.py:197-199 over the envs in global order.
Test infrastructure only.
"""
import numpy as np

from oracle import philox as P

BITS = 16
HASH_TAG = 0xFFFFFFFE
BETA = 0.1


def _popcount(x):
    x = np.asarray(x, np.uint32)
    return np.unpackbits(x.view(np.uint8).reshape(x.shape + (4,)), axis=-1).sum(axis=-1).astype(np.int64)


def matrix(D, seed):
    """(16, D) int8 hash matrix."""
    q = np.arange((D + 3) // 4, dtype=np.uint32)[None, :]
    b = np.arange(BITS, dtype=np.uint32)[:, None]
    w = P.philox4x32_10(q, b, np.uint32(0), np.uint32(HASH_TAG), seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    w = np.stack([np.broadcast_to(x, (BITS, q.shape[1])) for x in w], axis=-1).reshape(BITS, -1)[:, :D]
    a = _popcount(w & np.uint32(0xFFFF)) - _popcount(w >> np.uint32(16))
    return a.astype(np.int8)


def projections(obs, A8):
    """(n, 16) int64 sums of a[b, d] * obs[n, d] (obs: uint8, any trailing shape)."""
    x = np.asarray(obs)
    assert x.dtype == np.uint8
    return x.reshape(x.shape[0], -1).astype(np.int64) @ A8.astype(np.int64).T


def keys(obs, A8):
    """(n,) int32 keys: bit b set iff projection b > 0 (strict, as np.greater in buffer.py:194)."""
    bits = projections(obs, A8) > 0
    return (bits.astype(np.int64) << np.arange(BITS)).sum(axis=1).astype(np.int32)


def bonus(step_keys, table, beta=BETA):
    """buffer.py:197-199 for one step: for the envs in order, count[key] += 1 and the bonus is
    beta / sqrt(count[key]).  `table` (65,536 int64 counts) is advanced in place.  Returns
    (counts seen (n,) int64, bonus (n,) float64)."""
    cnt = np.empty(len(step_keys), np.int64)
    for i, k in enumerate(step_keys):
        table[k] += 1
        cnt[i] = table[k]
    return cnt, beta / np.sqrt(cnt.astype(np.float64))


def add_bonus(rewards, step_keys, table, beta=BETA):
    """rewards (n,) f32 -> f32(f64(rewards) + bonus), the reference's float64 add stored as f32."""
    _, bn = bonus(step_keys, table, beta)
    return (np.asarray(rewards, np.float32).astype(np.float64) + bn).astype(np.float32)


def new_table():
    return np.zeros(1 << BITS, np.int64)


def catch_stacks(n_envs, steps, seed, action_seed=None):
    """Random-policy Catch (tests/real_env_twin.py): (steps, n_envs, 4, 84, 84) uint8 stacks, the
    reset observation first."""
    from real_env_twin import CatchTwin, draw_actions
    tw = CatchTwin(n_envs, seed=seed)
    out = [tw.obs.copy()]
    for t in range(steps - 1):
        out.append(tw.step(draw_actions("Catch-v0", seed if action_seed is None else action_seed, tw.gids, t))["obs"])
    return np.stack(out)
