"""Numpy twin of the real-dynamics device envs (ppo-exploration_amd/csrc/env_real.hip).

Written from the equations of DESIGN.md "Real-dynamics envs" — the published gym
classic-control tasks restated (gym is not installed: parity with gym itself is unpinned) —
in float64 with numpy sin/cos, every operation in the order the kernels use, so the two
differ only in the last ulp of sin/cos.  Test infrastructure only.
"""
import math

import numpy as np

from oracle import philox as P

PI = math.pi
CARTPOLE, MOUNTAINCAR, ACROBOT, PENDULUM = 0, 1, 2, 3

# env id -> kind, state dim, obs dim, actions (count, or None for the Box((1,)) torque), max episode length
SPECS = {
    "CartPole-v1": (CARTPOLE, 4, 4, 2, 500),
    "CartPole-v0": (CARTPOLE, 4, 4, 2, 200),
    "MountainCar-v0": (MOUNTAINCAR, 2, 2, 3, 200),
    "Acrobot-v1": (ACROBOT, 4, 6, 3, 500),
    "Pendulum-v1": (PENDULUM, 2, 3, None, 200),
}
RESET_BOUNDS = {
    CARTPOLE: ([-0.05] * 4, [0.05] * 4),
    MOUNTAINCAR: ([-0.6, 0.0], [-0.4, 0.0]),
    ACROBOT: ([-0.1] * 4, [0.1] * 4),
    PENDULUM: ([-PI, -1.0], [PI, 1.0]),
}
EPS = 1e-12  # a flag may differ between twin and device only when a threshold quantity is this close


def _key(seed):
    return seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF


def reset_state(kind, seed, gids, episodes):
    """(n, S) f64: component j = lo_j + (hi_j - lo_j) * (double)u01(word_j) of
    philox({0, global env id, episode index, RESET_ACTION}, seed)."""
    k0, k1 = _key(seed)
    w = P.philox4x32_10(np.uint32(0), np.asarray(gids, np.uint32), np.asarray(episodes, np.uint32),
                        np.uint32(P.RESET_ACTION), k0, k1)
    lo, hi = (np.asarray(b, np.float64) for b in RESET_BOUNDS[kind])
    u = np.stack([P.u01(w[j]).astype(np.float64) for j in range(len(lo))], axis=-1)
    return lo + (hi - lo) * u


def wrap_pi(x):
    """((x + pi) mod 2pi) - pi, floored mod."""
    return np.mod(x + PI, 2 * PI) - PI


def _acrobot_dsdt(s, torque):
    m1 = m2 = l1 = 1.0
    lc1 = lc2 = 0.5
    I1 = I2 = 1.0
    g = 9.8
    th1, th2, dth1, dth2 = s[:, 0], s[:, 1], s[:, 2], s[:, 3]
    c2, s2 = np.cos(th2), np.sin(th2)
    d1 = m1 * lc1 * lc1 + m2 * (l1 * l1 + lc2 * lc2 + 2 * l1 * lc2 * c2) + I1 + I2
    d2 = m2 * (lc2 * lc2 + l1 * lc2 * c2) + I2
    phi2 = m2 * lc2 * g * np.cos(th1 + th2 - PI / 2)
    phi1 = (-m2 * l1 * lc2 * dth2 * dth2 * s2 - 2 * m2 * l1 * lc2 * dth2 * dth1 * s2
            + (m1 * lc1 + m2 * l1) * g * np.cos(th1 - PI / 2) + phi2)
    ddth2 = (torque + d2 / d1 * phi1 - m2 * l1 * lc2 * dth1 * dth1 * s2 - phi2) / (m2 * lc2 * lc2 + I2 - d2 * d2 / d1)
    ddth1 = -(d2 * ddth2 + phi1) / d1
    return np.stack([dth1, dth2, ddth1, ddth2], axis=-1)


def physics(kind, state, actions):
    """One step from `state` (n, S) f64 -> (next state, reward f64, terminated, near): `near` marks the
    envs where a quantity that decides a flag or a branch lies within EPS of its threshold."""
    s = np.array(state, np.float64)
    n = s.shape[0]
    near = np.zeros(n, bool)
    if kind == CARTPOLE:
        a = np.asarray(actions).reshape(n)
        x, xd, th, thd = s[:, 0], s[:, 1], s[:, 2], s[:, 3]
        f = np.where(a == 1, 10.0, -10.0)
        cth, sth = np.cos(th), np.sin(th)
        temp = (f + 0.05 * thd * thd * sth) / 1.1
        tha = (9.8 * sth - cth * temp) / (0.5 * (4.0 / 3.0 - 0.1 * cth * cth / 1.1))
        xa = temp - 0.05 * tha * cth / 1.1
        x = x + 0.02 * xd
        xd = xd + 0.02 * xa
        th = th + 0.02 * thd
        thd = thd + 0.02 * tha
        lim = 12 * 2 * PI / 360
        term = (np.abs(x) > 2.4) | (np.abs(th) > lim)
        near = (np.abs(np.abs(x) - 2.4) < EPS) | (np.abs(np.abs(th) - lim) < EPS)
        return np.stack([x, xd, th, thd], axis=-1), np.ones(n), term, near
    if kind == MOUNTAINCAR:
        a = np.asarray(actions).reshape(n).astype(np.int64)
        p, v = s[:, 0], s[:, 1]
        v = v + ((a - 1).astype(np.float64) * 0.001 + np.cos(3 * p) * (-0.0025))
        v = np.clip(v, -0.07, 0.07)
        p_free = p + v
        p = np.clip(p_free, -1.2, 0.6)
        wall = (p == -1.2) & (v < 0)
        near = (np.abs(p_free + 1.2) < EPS) & (v < 0)
        v = np.where(wall, 0.0, v)
        term = (p >= 0.5) & (v >= 0)
        near |= ((np.abs(p - 0.5) < EPS) & (v > -EPS)) | ((np.abs(v) < EPS) & (p > 0.5 - EPS))
        return np.stack([p, v], axis=-1), -np.ones(n), term, near
    if kind == ACROBOT:
        torque = (np.asarray(actions).reshape(n).astype(np.int64) - 1).astype(np.float64)
        dt = 0.2
        dt2 = dt / 2
        k1 = _acrobot_dsdt(s, torque)
        k2 = _acrobot_dsdt(s + dt2 * k1, torque)
        k3 = _acrobot_dsdt(s + dt2 * k2, torque)
        k4 = _acrobot_dsdt(s + dt * k3, torque)
        s = s + dt / 6.0 * (k1 + 2 * k2 + 2 * k3 + k4)
        for j in (0, 1):
            r = np.mod(s[:, j] + PI, 2 * PI)
            near |= (r < EPS) | (2 * PI - r < EPS)
            s[:, j] = r - PI
        s[:, 2] = np.clip(s[:, 2], -4 * PI, 4 * PI)
        s[:, 3] = np.clip(s[:, 3], -9 * PI, 9 * PI)
        height = -np.cos(s[:, 0]) - np.cos(s[:, 0] + s[:, 1])
        term = height > 1.0
        near |= np.abs(height - 1.0) < EPS
        return s, np.where(term, 0.0, -1.0), term, near
    if kind == PENDULUM:
        th, thd = s[:, 0], s[:, 1]
        u = np.clip(np.asarray(actions, np.float32).reshape(n).astype(np.float64), -2.0, 2.0)
        w = wrap_pi(th)
        cost = w * w + 0.1 * thd * thd + 0.001 * u * u
        nthd = np.clip(thd + (15.0 * np.sin(th) + 3.0 * u) * 0.05, -8.0, 8.0)
        return np.stack([th + nthd * 0.05, nthd], axis=-1), -cost, np.zeros(n, bool), near
    raise ValueError(kind)


def observe(kind, state):
    s = np.asarray(state, np.float64)
    if kind in (CARTPOLE, MOUNTAINCAR):
        return s.astype(np.float32)
    if kind == ACROBOT:
        cols = [np.cos(s[:, 0]), np.sin(s[:, 0]), np.cos(s[:, 1]), np.sin(s[:, 1]), s[:, 2], s[:, 3]]
    else:
        cols = [np.cos(s[:, 0]), np.sin(s[:, 0]), s[:, 1]]
    return np.stack(cols, axis=-1).astype(np.float32)


class ControlTwin:
    """The device env's step, auto-reset and episode bookkeeping.  `state`, `episode`, `ep_ret` and
    `ep_len` are plain arrays: a teacher-forced test overwrites them with the device's before a step."""

    def __init__(self, env_id, n_envs, seed=0, env_offset=0, max_len=None):
        self.kind, self.s_dim, self.obs_dim, self.n_actions, ml = SPECS[env_id]
        self.num_envs, self.seed = n_envs, seed
        self.gids = np.arange(env_offset, env_offset + n_envs)
        self.max_len = ml if max_len is None else max_len
        self.reset()

    def reset(self):
        n = self.num_envs
        self.episode = np.zeros(n, np.int32)
        self.state = reset_state(self.kind, self.seed, self.gids, self.episode)
        self.ep_ret = np.zeros(n, np.float32)
        self.ep_len = np.zeros(n, np.int32)
        return observe(self.kind, self.state)

    def step(self, actions):
        """-> dict(obs f32, reward f32, reward64, done, terminated, near, done_ret, done_len, pre_reset_state)."""
        s, r64, term, near = physics(self.kind, self.state, actions)
        done = term | (self.ep_len + 1 >= self.max_len)
        rew = r64.astype(np.float32)
        ret = (self.ep_ret + rew).astype(np.float32)
        ln = self.ep_len + 1
        done_ret = np.where(done, ret, np.float32(np.nan)).astype(np.float32)
        done_len = np.where(done, ln, 0).astype(np.int32)
        self.ep_ret = np.where(done, np.float32(0), ret).astype(np.float32)
        self.ep_len = np.where(done, 0, ln).astype(np.int32)
        self.episode = (self.episode + done).astype(np.int32)
        fresh = reset_state(self.kind, self.seed, self.gids, self.episode)
        self.state = np.where(done[:, None], fresh, s)
        return dict(obs=observe(self.kind, self.state), reward=rew, reward64=r64, done=done, terminated=term,
                    near=near, done_ret=done_ret, done_len=done_len, pre_reset_state=s)


# ------------------------------------------------------------------------------------------ Catch
GRID, CELL = 12, 7


def catch_reset_state(seed, gids, episodes):
    """(n, 4) int32 = ball column, ball row, ball dx, paddle column from
    philox({EVENT_BLOCK, global env id, episode index, RESET_ACTION}, seed)."""
    k0, k1 = _key(seed)
    w = P.philox4x32_10(np.uint32(P.EVENT_BLOCK), np.asarray(gids, np.uint32), np.asarray(episodes, np.uint32),
                        np.uint32(P.RESET_ACTION), k0, k1)
    col = (w[0] % np.uint32(GRID)).astype(np.int32)
    dx = (w[1] % np.uint32(3)).astype(np.int32) - 1
    pad = 1 + (w[2] % np.uint32(10)).astype(np.int32)
    return np.stack([col, np.zeros_like(col), dx, pad], axis=-1).astype(np.int32)


def catch_frame(state):
    """(n, 84, 84) uint8: zeros, the three paddle cells (bottom row) 128, the ball cell 255."""
    n = state.shape[0]
    cells = np.zeros((n, GRID, GRID), np.uint8)
    for i in range(n):
        col, row, _, pad = (int(v) for v in state[i])
        cells[i, GRID - 1, pad - 1:pad + 2] = 128
        cells[i, row, col] = 255
    return np.repeat(np.repeat(cells, CELL, axis=1), CELL, axis=2)


def catch_physics(state, actions):
    """-> (next state before any reset, reward f32, done)."""
    s = np.array(state, np.int64)
    a = np.asarray(actions).reshape(-1).astype(np.int64)
    col, row, dx, pad = s[:, 0], s[:, 1], s[:, 2], s[:, 3]
    pad = np.clip(pad + np.where(a == 1, -1, np.where(a == 2, 1, 0)), 1, GRID - 2)
    row = row + 1
    col = col + dx
    low, high = col < 0, col > GRID - 1
    col = np.where(low, -col, np.where(high, 2 * (GRID - 1) - col, col))
    dx = np.where(low | high, -dx, dx)
    done = row == GRID - 1
    rew = np.where(done, np.where(np.abs(col - pad) <= 1, 1.0, -1.0), 0.0).astype(np.float32)
    return np.stack([col, row, dx, pad], axis=-1).astype(np.int32), rew, done


class CatchTwin:
    def __init__(self, n_envs, seed=0, env_offset=0):
        self.num_envs, self.seed = n_envs, seed
        self.gids = np.arange(env_offset, env_offset + n_envs)
        self.reset()

    def reset(self):
        n = self.num_envs
        self.episode = np.zeros(n, np.int32)
        self.state = catch_reset_state(self.seed, self.gids, self.episode)
        self.ep_ret = np.zeros(n, np.float32)
        self.ep_len = np.zeros(n, np.int32)
        self.obs = np.zeros((n, 4, 84, 84), np.uint8)
        self.obs[:, 3] = catch_frame(self.state)
        return self.obs.copy()

    def step(self, actions):
        s, rew, done = catch_physics(self.state, actions)
        ret = (self.ep_ret + rew).astype(np.float32)
        ln = self.ep_len + 1
        done_ret = np.where(done, ret, np.float32(np.nan)).astype(np.float32)
        done_len = np.where(done, ln, 0).astype(np.int32)
        self.ep_ret = np.where(done, np.float32(0), ret).astype(np.float32)
        self.ep_len = np.where(done, 0, ln).astype(np.int32)
        self.episode = (self.episode + done).astype(np.int32)
        self.state = np.where(done[:, None], catch_reset_state(self.seed, self.gids, self.episode), s)
        nxt = np.empty_like(self.obs)
        nxt[:, :3] = self.obs[:, 1:]
        nxt[done, :3] = 0
        nxt[:, 3] = catch_frame(self.state)
        self.obs = nxt
        return dict(obs=nxt.copy(), reward=rew, done=done, done_ret=done_ret, done_len=done_len)


# ---------------------------------------------------------------------- test actions (Philox-keyed)
# the shape of the GPU parity run (test_real_env_gpu.py); test_real_env_twin.py checks on the CPU that the
# twin's own run with this seed stays clear of every threshold
PARITY_N, PARITY_T, PARITY_SEED = 67, 64, 20
ACTION_STREAM = 0x0AC710  # counter word that keeps the tests' action draws apart from the envs' own


def draw_actions(env_id, seed, gids, t):
    """The tests' actions at step t for global env ids `gids`: integers below the action count, or
    float32 torques uniform in [-2.5, 2.5) for Pendulum (so the clip to +-2 is exercised)."""
    k0, k1 = _key(seed)
    w = P.philox4x32_10(np.uint32(t), np.asarray(gids, np.uint32), np.uint32(ACTION_STREAM), np.uint32(0), k0, k1)
    n_actions = 3 if env_id == "Catch-v0" else SPECS[env_id][3]
    if n_actions is None:
        return (P.u01(w[0]) * np.float32(5.0) - np.float32(2.5)).astype(np.float32).reshape(-1, 1)
    return (w[0] % np.uint32(n_actions)).astype(np.int32)

