"""Numpy twin of the ES episode kernel on the real-dynamics control tasks (es_eval_control_kernel in
ppo-exploration_amd/csrc/es.hip, entry point ppox_es_evaluate_control): test helper, not a test module.
tests/test_es_control_twin.py checks it on the CPU, tests/test_es_control_gpu.py holds the kernel to it.

Written from the entry point's paragraph in include/ppox.h on real_env_twin.reset_state / observe / physics.

  Start     reset_state(kind, env_seed, gid 0, episode): every member of a call starts from the same state.
  Step t    obs = observe(state) (float32) widened to float64;
            layer 0   acc = 0; acc = acc + obs[i] * W0[i, l] for i = 0 .. D-1 in order;  h1 = arctan(acc)
            layer 1   four chains c0..c3, chain k % 4 taking h1[k] * W1[k, l] for k = 0 .. H1-1 in order, summed
                      (c0 + c1) + (c2 + c3);  h2 = arctan(.)
            head      z_j = the 64-lane butterfly sum of h2[l] * W2[l, j] (lanes >= H2 hold 0): six rounds
                      v[l] = v[l] + v[l ^ o] for o = 32, 16, 8, 4, 2, 1
            The kernel's layer 1 is a fused multiply-add per term; numpy has none, so the twin rounds the product
            first.  That moves z by a few 1e-16: decisions are compared only where `margin` is >= 1e-9.
            Discrete  p_j = exp(z_j - max z), S = p_0 + p_1 (+ p_2) in order, q_j = p_j / S,
                      u = float64(u01(first word of philox({t, member0 + p, episode, ACT_TAG}, env_seed))),
                      action = the first j < A-1 with u < q_0 + .. + q_j (running sum in order), else A-1
            Pendulum  torque = float32(2 * tanh(z_0))
            then physics(state, action); fitness += reward; steps += 1; the member stops when terminated.

`episodes` returns per member: fitness, steps, bc (the final state[0:2]), the actions (the entries at steps not
taken stay at ACTION_FILL / NaN), `margin` = the smallest |u - (q_0 + .. + q_j)| over the steps taken (inf for
Pendulum), and `near` = the OR of physics' `near` over the steps taken.  With `actions` given it replays them
instead of deciding (teacher-forced: the device's own decisions through the twin's physics).

`episodes_ld` is the same function in np.longdouble (80-bit x87) for Pendulum and Acrobot, as es_twin.evaluate_ld:
the float64 constants are the kernel's own doubles widened, the float32 roundings of the observation and of the
torque stay, only the arithmetic in between is wider.  PENDULUM_TOL comes from it."""
import math

import numpy as np

import real_env_twin as R
from oracle import philox as P

LD = np.longdouble
ACT_TAG = 0xAC7AC7AC      # include/ppox.h PPOX_ES_ACT_TAG
ACTION_FILL = -1          # twin's marker for an action slot at a step not taken
MARGIN = 1e-9             # decisions are compared where the draw is at least this far from every threshold

KINDS = {"CartPole-v1": R.CARTPOLE, "MountainCar-v0": R.MOUNTAINCAR, "Acrobot-v1": R.ACROBOT,
         "Pendulum-v1": R.PENDULUM}
OBS_DIM = {R.CARTPOLE: 4, R.MOUNTAINCAR: 2, R.ACROBOT: 6, R.PENDULUM: 3}
N_ACT = {R.CARTPOLE: 2, R.MOUNTAINCAR: 3, R.ACROBOT: 3, R.PENDULUM: 1}

# the shape table of the per-kind tests
ENV_SEED = (0x9E3779B9 << 32) | 0x7F4A7C15  # a non-zero high key word
EPISODE = 3
SIGMA = 0.1
POPS = (1, 5, 257)          # a lone wave, a block with an idle wave, many blocks
HIDDEN = ((1, 1), (3, 7), (64, 64))
LENGTHS = (1, 2, 40)

# Pendulum has continuous feedback, so nothing can be teacher-forced: the kernel's free run is held to
# 16 x the float64 twin's own worst distance from episodes_ld over the Pendulum cases at T = 40 (fitness, bc and
# torques, relative to max(1, |value|)).  Measured on the CPU (test_es_control_twin.py recomputes it):
# 1.095e-13, on the behaviour at (3, 7), P = 257, eps given; the fitness (a sum of 40 float32 rewards, exact in
# float64) and the float32 torques agree exactly.  Written here rounded up to 1.2e-13: the run amplifies the
# last ulp of numpy's sin / cos / arctan about a thousandfold, so another libm moves the figure by a few percent.
PENDULUM_TWIN_WORST = 1.2e-13
PENDULUM_TOL = 16 * PENDULUM_TWIN_WORST
# the bound test_real_env_gpu.py holds per step, here on the replayed episode at T <= 40
REPLAY_TOL = 1e-12


def ld_ok():
    return np.finfo(LD).eps < 1e-18


LD_SKIP_REASON = "np.longdouble is no wider than float64 here: no high-precision reference"


def sizes(kind, hidden):
    return [OBS_DIM[kind], hidden[0], hidden[1], N_ACT[kind]]


def n_params(kind, hidden):
    s = sizes(kind, hidden)
    return int(sum(a * b for a, b in zip(s[:-1], s[1:])))


def case_weights(kind, hidden):
    """[W0 (D, H1), W1 (H1, H2), W2 (H2, A)] float64, randn / sqrt(fan_in), one fixed draw per (kind, hidden)"""
    s = sizes(kind, hidden)
    rs = np.random.RandomState(kind * 100003 + hidden[0] * 1009 + hidden[1])
    return [rs.randn(a, b) / np.sqrt(a) for a, b in zip(s[:-1], s[1:])]


def case_eps(kind, hidden, n_members):
    """(n_members, n_params) float64 standard normal, one fixed draw per case"""
    rs = np.random.RandomState(7 + kind * 100003 + hidden[0] * 1009 + hidden[1] + 31 * n_members)
    return rs.randn(n_members, n_params(kind, hidden))


def flat(weights):
    return np.concatenate([np.asarray(w).reshape(-1) for w in weights])


def members(weights, eps, sigma, n_members=None):
    """theta_p = w + sigma * eps_p per layer as the kernel forms it (eps None: n_members copies of w)"""
    if eps is None:
        return [[np.array(w, np.float64) for w in weights] for _ in range(n_members or 1)]
    out = []
    for row in np.asarray(eps, np.float64):
        off, ws = 0, []
        for w in weights:
            ws.append(w + sigma * row[off:off + w.size].reshape(w.shape))
            off += w.size
        out.append(ws)
    return out


def _key(seed):
    return seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF


def action_uniform(env_seed, t, member_ids, episode):
    k0, k1 = _key(env_seed)
    w = P.philox4x32_10(np.uint32(t), np.asarray(member_ids, np.uint64).astype(np.uint32), np.uint32(episode),
                        np.uint32(ACT_TAG), k0, k1)
    return P.u01(w[0]).astype(np.float64)


def logits(obs, W0, W1, W2):
    """obs (M, D), W0 (M, D, H1), W1 (M, H1, H2), W2 (M, H2, A) of one dtype -> z (M, A), in the kernel's orders"""
    M, D, H1 = W0.shape
    H2, A = W2.shape[1:]
    dt = W0.dtype
    acc = np.zeros((M, H1), dt)
    for i in range(D):
        acc = acc + obs[:, i:i + 1] * W0[:, i, :]
    h1 = np.arctan(acc)
    c = [np.zeros((M, H2), dt) for _ in range(4)]
    for k in range(H1):
        c[k % 4] = c[k % 4] + h1[:, k:k + 1] * W1[:, k, :]
    h2 = np.arctan((c[0] + c[1]) + (c[2] + c[3]))
    lanes = np.arange(64)
    z = np.empty((M, A), dt)
    for j in range(A):
        v = np.zeros((M, 64), dt)
        v[:, :H2] = h2 * W2[:, :, j]
        for o in (32, 16, 8, 4, 2, 1):
            v = v + v[:, lanes ^ o]
        z[:, j] = v[:, 0]
    return z


def decide(z, u):
    """z (M, A) float64, u (M,) -> (action int32 (M,), margin (M,)): the softmax inverse CDF of the kernel"""
    M, A = z.shape
    m = z.max(axis=1)
    p = np.exp(z - m[:, None])
    S = p[:, 0]
    for j in range(1, A):
        S = S + p[:, j]
    q = p / S[:, None]
    a = np.full(M, A - 1, np.int32)
    found = np.zeros(M, bool)
    margin = np.full(M, np.inf)
    c = np.zeros(M)
    for j in range(A - 1):
        c = c + q[:, j]
        hit = ~found & (u < c)
        a[hit] = j
        found |= hit
        margin = np.minimum(margin, np.abs(u - c))
    return a, margin


def _stack(weights_list, dtype):
    return [np.stack([np.asarray(ws[i], np.float64) for ws in weights_list]).astype(dtype) for i in range(3)]


def episodes(kind, weights_list, T, env_seed, episode, member0=0, actions=None, trace=False):
    """-> dict(fitness (M,), steps (M,) int32, bc (M, 2), actions (M, T), margin (M,), near (M,)
    [, states (M, T, S) after each step taken, rewards (M, T)]).  weights_list may be None when `actions` is given
    (M = len(actions))."""
    M = len(actions) if weights_list is None else len(weights_list)
    pend = kind == R.PENDULUM
    if weights_list is not None:
        W0, W1, W2 = _stack(weights_list, np.float64)
    s = np.repeat(R.reset_state(kind, env_seed, [0], [episode]), M, axis=0)
    alive = np.ones(M, bool)
    fit = np.zeros(M)
    steps = np.zeros(M, np.int32)
    margin = np.full(M, np.inf)
    near = np.zeros(M, bool)
    acts = np.full((M, T), np.nan, np.float32) if pend else np.full((M, T), ACTION_FILL, np.int32)
    states = np.full((M, T, s.shape[1]), np.nan)
    rewards = np.full((M, T), np.nan)
    ids = member0 + np.arange(M, dtype=np.int64)
    for t in range(T):
        if not alive.any():
            break
        if actions is not None:
            a = np.asarray(actions)[:, t]
        else:
            z = logits(R.observe(kind, s).astype(np.float64), W0, W1, W2)
            if pend:
                a = (2.0 * np.tanh(z[:, 0])).astype(np.float32)
            else:
                a, mg = decide(z, action_uniform(env_seed, t, ids, episode))
                margin = np.where(alive, np.minimum(margin, mg), margin)
        acts[alive, t] = a[alive]
        s2, rew, term, nr = R.physics(kind, s, a)
        s = np.where(alive[:, None], s2, s)
        fit = np.where(alive, fit + rew.astype(np.float32).astype(np.float64), fit)
        steps = steps + alive
        near |= alive & nr
        states[alive, t] = s[alive]
        rewards[alive, t] = rew[alive]
        alive = alive & ~term
    out = dict(fitness=fit, steps=steps.astype(np.int32), bc=s[:, :2].copy(), actions=acts, margin=margin, near=near)
    if trace:
        out.update(states=states, rewards=rewards)
    return out


# ------------------------------------------------------------------------------------------ long double
PI_LD = LD(math.pi)  # the kernel's double pi, widened


def _wrap_pi_ld(x):
    return np.mod(x + PI_LD, LD(2) * PI_LD) - PI_LD


def _acrobot_dsdt_ld(s, torque):
    g, half = LD(9.8), LD(0.5)
    th1, th2, dth1, dth2 = s[:, 0], s[:, 1], s[:, 2], s[:, 3]
    c2, s2 = np.cos(th2), np.sin(th2)
    d1 = half * half + (LD(1) + half * half + LD(2) * half * c2) + LD(1) + LD(1)
    d2 = (half * half + half * c2) + LD(1)
    phi2 = half * g * np.cos(th1 + th2 - PI_LD / LD(2))
    phi1 = (-half * dth2 * dth2 * s2 - LD(2) * half * dth2 * dth1 * s2
            + (half + LD(1)) * g * np.cos(th1 - PI_LD / LD(2)) + phi2)
    ddth2 = (torque + d2 / d1 * phi1 - half * dth1 * dth1 * s2 - phi2) / (half * half + LD(1) - d2 * d2 / d1)
    ddth1 = -(d2 * ddth2 + phi1) / d1
    return np.stack([dth1, dth2, ddth1, ddth2], axis=-1)


def _physics_ld(kind, s, a):
    """real_env_twin.physics for Pendulum and Acrobot in long double -> (state, reward, terminated)"""
    n = s.shape[0]
    if kind == R.PENDULUM:
        th, thd = s[:, 0], s[:, 1]
        u = np.clip(np.asarray(a, np.float32).astype(LD), LD(-2), LD(2))
        w = _wrap_pi_ld(th)
        cost = w * w + LD(0.1) * thd * thd + LD(0.001) * u * u
        nthd = np.clip(thd + (LD(15.0) * np.sin(th) + LD(3.0) * u) * LD(0.05), LD(-8), LD(8))
        return np.stack([th + nthd * LD(0.05), nthd], axis=-1), -cost, np.zeros(n, bool)
    if kind == R.ACROBOT:
        torque = (np.asarray(a).astype(np.int64) - 1).astype(LD)
        dt = LD(0.2)
        dt2 = dt / LD(2)
        k1 = _acrobot_dsdt_ld(s, torque)
        k2 = _acrobot_dsdt_ld(s + dt2 * k1, torque)
        k3 = _acrobot_dsdt_ld(s + dt2 * k2, torque)
        k4 = _acrobot_dsdt_ld(s + dt * k3, torque)
        s = s + dt / LD(6.0) * (k1 + LD(2) * k2 + LD(2) * k3 + k4)
        s[:, 0] = _wrap_pi_ld(s[:, 0])
        s[:, 1] = _wrap_pi_ld(s[:, 1])
        s[:, 2] = np.clip(s[:, 2], LD(-4) * PI_LD, LD(4) * PI_LD)
        s[:, 3] = np.clip(s[:, 3], LD(-9) * PI_LD, LD(9) * PI_LD)
        term = -np.cos(s[:, 0]) - np.cos(s[:, 0] + s[:, 1]) > LD(1)
        return s, np.where(term, LD(0), LD(-1)), term
    raise ValueError("the long-double restatement covers Pendulum and Acrobot")


def _observe_ld(kind, s):
    if kind == R.ACROBOT:
        cols = [np.cos(s[:, 0]), np.sin(s[:, 0]), np.cos(s[:, 1]), np.sin(s[:, 1]), s[:, 2], s[:, 3]]
    else:
        cols = [np.cos(s[:, 0]), np.sin(s[:, 0]), s[:, 1]]
    return np.stack(cols, axis=-1).astype(np.float32).astype(LD)


def episodes_ld(kind, weights_list, T, env_seed, episode, actions=None):
    """`episodes` in long double (Pendulum: free run; Acrobot: the given actions replayed) -> dict(fitness, bc,
    actions, steps), fitness and bc as np.longdouble."""
    if not ld_ok():
        raise RuntimeError(LD_SKIP_REASON)
    pend = kind == R.PENDULUM
    M = len(actions) if weights_list is None else len(weights_list)
    if weights_list is not None:
        W0, W1, W2 = _stack(weights_list, LD)
    s = np.repeat(R.reset_state(kind, env_seed, [0], [episode]), M, axis=0).astype(LD)
    alive = np.ones(M, bool)
    fit = np.zeros(M, LD)
    steps = np.zeros(M, np.int32)
    acts = np.full((M, T), np.nan, np.float32)
    for t in range(T):
        if not alive.any():
            break
        if actions is not None:
            a = np.asarray(actions)[:, t]
        else:
            z = logits(_observe_ld(kind, s), W0, W1, W2)
            a = (LD(2) * np.tanh(z[:, 0])).astype(np.float32)
        acts[alive, t] = a[alive]
        s2, rew, term = _physics_ld(kind, s, a)
        s = np.where(alive[:, None], s2, s)
        r = rew.astype(np.float32).astype(LD) if pend else rew
        fit = np.where(alive, fit + r, fit)
        steps = steps + alive
        alive = alive & ~term
    return dict(fitness=fit, bc=s[:, :2].copy(), actions=acts, steps=steps.astype(np.int32))


def rel_err(got, ref):
    """max |got - ref| / max(1, |ref|), in long double"""
    got, ref = np.asarray(got, LD), np.asarray(ref, LD)
    return float(np.max(np.abs(got - ref) / np.maximum(LD(1), np.abs(ref))))


def case_inputs(kind, hidden, n_members, with_eps):
    """(weights, eps or None, members) of one per-kind case"""
    w = case_weights(kind, hidden)
    eps = case_eps(kind, hidden, n_members) if with_eps else None
    return w, eps, members(w, eps, SIGMA, n_members)


# the constructed MountainCar policy: push the way the car is moving (h1 = atan(1e4 v) is +-pi/2 off rest,
# h2 = atan(h1) about +-1, logits -+40, 0, +-40); from rest the logits are 0 and the first push is drawn uniformly
def mountaincar_policy():
    return [np.array([[0.0], [1e4]]), np.array([[1.0]]), np.array([[-40.0, 0.0, 40.0]])]
