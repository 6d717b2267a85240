"""Numpy twins of the synthetic device envs' missing pieces (csrc/env.hip, csrc/episode.h): test
helper, not a test module.  Built on oracle.philox (philox4x32_10, u01, events, SyntheticAtari),
which stays as it is; tests/test_synth_env_twin.py checks this file on the CPU and
tests/test_synth_env_gpu.py holds the kernels to it.  Everything here is integers, float32 values
k / 2^24 and sums of ones: the comparison with the device is exact.

  Episode         the bookkeeping of episode.h: ep_ret, ep_len, and the record of the episode that ended at
                  this step, done_ret (NaN when none did) and done_len (0 when none did)
  SyntheticVec    vec_step_kernel: obs word 4b + j of counter (b, global env, step, a) -> u01 * 2 - 1; a is the
                  action (Discrete), 0 (Box: actions == nullptr) or RESET_ACTION at step 0 (reset); reward 1;
                  done = u01(ev.y) < p_done or (max_len > 0 and ep_len + 1 >= max_len), ev the EVENT_BLOCK draw
  AtariEpisodes   oracle.philox.SyntheticAtari with the Episode bookkeeping round it"""
import numpy as np

from oracle import philox as PH


class Episode:
    """episode_update of csrc/episode.h over all envs at once (float32 return, int32 length)."""

    def ep_reset(self, n):
        self.ep_ret = np.zeros(n, np.float32)
        self.ep_len = np.zeros(n, np.int32)
        self.done_ret = np.full(n, np.nan, np.float32)
        self.done_len = np.zeros(n, np.int32)

    def ep_update(self, rew, done):
        done = np.asarray(done, bool)
        r = (self.ep_ret + np.asarray(rew, np.float32)).astype(np.float32)
        ln = (self.ep_len + 1).astype(np.int32)
        self.done_ret = np.where(done, r, np.float32(np.nan)).astype(np.float32)
        self.done_len = np.where(done, ln, 0).astype(np.int32)
        self.ep_ret = np.where(done, np.float32(0), r).astype(np.float32)
        self.ep_len = np.where(done, 0, ln).astype(np.int32)


def as_u32(actions, n):
    """int32 actions as the kernel reads them: (uint32_t)actions[n]"""
    return (np.asarray(actions).astype(np.int64).reshape(n) & 0xFFFFFFFF).astype(np.uint32)


def vec_obs(seed, env_ids, step, actions, D):
    """(n, D) float32: word j of Philox block b at counter (b, env, step, action) is obs[4b + j]."""
    k0, k1 = PH._key(seed)
    gid = np.asarray(env_ids, np.uint32)[:, None]
    a = np.asarray(actions, np.uint32)[:, None]
    blocks = np.arange((D + 3) // 4, dtype=np.uint32)[None, :]
    w = np.stack(PH.philox4x32_10(blocks, gid, np.uint32(step), a, k0, k1), axis=-1)  # (n, blocks, 4)
    return PH.u01(w.reshape(len(gid), -1)[:, :D]) * np.float32(2) - np.float32(1)


class SyntheticVec(Episode):
    def __init__(self, n_envs, obs_dim, seed, p_done=0.0, max_len=0, env_offset=0, discrete=True):
        self.num_envs, self.obs_dim, self.seed = n_envs, obs_dim, seed
        self.p_done, self.max_len, self.discrete = p_done, max_len, discrete
        self.env_ids = np.arange(env_offset, env_offset + n_envs)
        self.k = 0
        self.ep_reset(n_envs)

    def reset(self):
        self.k = 0
        self.ep_reset(self.num_envs)
        return vec_obs(self.seed, self.env_ids, 0, np.full(self.num_envs, PH.RESET_ACTION, np.uint32), self.obs_dim)

    def step(self, actions=None):
        """-> obs (n, D) f32, rewards (n,) f32, dones (n,) bool; the episode arrays are attributes"""
        self.k += 1
        n = self.num_envs
        a = as_u32(actions, n) if (self.discrete and actions is not None) else np.zeros(n, np.uint32)
        obs = vec_obs(self.seed, self.env_ids, self.k, a, self.obs_dim)
        _, rnd = PH.events(self.seed, self.env_ids, self.k, a, 0.0, self.p_done)
        done = rnd | ((self.max_len > 0) & (self.ep_len + 1 >= self.max_len))
        rew = np.ones(n, np.float32)
        self.ep_update(rew, done)
        return obs, rew, done


class AtariEpisodes(Episode):
    def __init__(self, *args, **kw):
        self.env = PH.SyntheticAtari(*args, **kw)
        self.ep_reset(self.env.num_envs)

    def reset(self):
        self.ep_reset(self.env.num_envs)
        return self.env.reset()

    def step(self, actions):
        obs, rew, done, infos = self.env.step(actions)
        self.ep_update(rew, done)
        return obs, rew, done, infos


def episode_infos(done_ret, done_len):
    """env.episode_infos on the twin's arrays"""
    return [{"episode": {"r": float(r), "l": int(ln)}} if not np.isnan(r) else {} for r, ln in zip(done_ret, done_len)]
