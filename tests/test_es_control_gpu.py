"""ppox_es_evaluate_control (csrc/es.hip es_eval_control_kernel): ES episodes on the real-dynamics control tasks,
against tests/es_control_twin.py (checked on the CPU by tests/test_es_control_twin.py).  Every buffer the kernel
writes is a view into a sentinel-filled allocation (tests/guarded.py), pre-filled with NaN or left at the sentinel.

Where each check comes from:
  decisions   the kernel's arctan / exp / fma move a logit by a few 1e-16, so on every member whose draws all lie
              at least MARGIN = 1e-9 from their thresholds (and whose physics flags are not within 1e-12 of
              flipping) the actions, the step count and the Discrete fitness are the twin's exactly.  At most one
              member of a case may fall outside; on the CPU the twin leaves out none.
  physics     the twin's physics replayed on the device's own actions: bc, steps and fitness within
              REPLAY_TOL = 1e-12 max(1, |x|), the bound test_real_env_gpu.py holds per step (sin / cos differ in the
              last ulp; measured here: see the printed figures).
  Pendulum    continuous feedback, nothing to teacher-force: fitness, bc and torques within PENDULUM_TOL = 16 x the
              float64 twin's own worst distance from its long-double restatement.
Everything else is bitwise equality between launches of the same kernel."""
import functools

import numpy as np
import pytest
import torch

import es_control_twin as C
import real_env_twin as R
from guarded import SENTINEL, Arena

pytestmark = pytest.mark.gpu
needs_ld = pytest.mark.skipif(not C.ld_ok(), reason=C.LD_SKIP_REASON)

NAN = float("nan")
F64, I32, F32 = torch.float64, torch.int32, torch.float32
SENT_I32 = int(np.array([SENTINEL] * 4, np.uint8).view(np.int32)[0])
DISCRETE = [e for e, k in C.KINDS.items() if k != R.PENDULUM]


def _native():
    import native
    return native


def _np(t):
    return t.cpu().numpy()


def _launch(kind, w, eps, n, hidden, T, member0=0, episode=C.EPISODE, env_seed=C.ENV_SEED, outputs=(1, 1, 1)):
    """One guarded launch -> dict of device tensors (fitness, steps, bc, actions) and the arena.  eps: numpy
    (n, n_params) or None; it is followed by three more rows of sentinel, which a block's idle waves that lost
    their early return would read instead of memory the test does not own."""
    arena = Arena()
    npar = C.n_params(kind, hidden)
    wd = arena.new(npar, F64, init=C.flat(w))
    ed = None if eps is None else arena.new((n, npar), F64, init=eps, guard=max(64, 3 * npar))
    fit = arena.new(n, F64, init=NAN)
    steps = arena.new(n, I32) if outputs[0] else None
    bc = arena.new((n, 2), F64, init=NAN) if outputs[1] else None
    acts = arena.new((n, T), I32) if outputs[2] else None  # int32 view of the sentinel bytes; f32 for Pendulum
    _native().es_evaluate_control(kind, wd, ed, C.SIGMA, n, member0, hidden[0], hidden[1], T, env_seed, episode, fit,
                                  steps, bc, acts)
    arena.check()
    return dict(fitness=fit, steps=steps, bc=bc, actions=acts, arena=arena)


def _actions_np(kind, acts):
    a = _np(acts)
    return a.view(np.float32) if kind == R.PENDULUM else a


def _untouched_past_the_end(kind, acts_i32, steps):
    """entries of actions_out at steps not taken still hold the sentinel"""
    T = acts_i32.shape[1]
    past = np.arange(T)[None, :] >= steps[:, None]
    assert (acts_i32[past] == SENT_I32).all()
    assert (acts_i32[~past] != SENT_I32).all()


@functools.lru_cache(maxsize=None)
def _case(env_id, hidden, n, T, with_eps):
    kind = C.KINDS[env_id]
    w, eps, mem = C.case_inputs(kind, hidden, n, with_eps)
    dev = _launch(kind, w, eps, n, hidden, T)
    twin = C.episodes(kind, mem, T, C.ENV_SEED, C.EPISODE)
    return kind, mem, dev, twin


def _check_discrete(kind, dev, twin, T, label):
    """decisions exactly on the members clear of every threshold, then the physics replayed on the device's
    actions; returns the number of members left out"""
    fit, steps, bc = _np(dev["fitness"]), _np(dev["steps"]), _np(dev["bc"])
    acts = _np(dev["actions"])
    n = len(fit)
    assert np.isfinite(fit).all() and np.isfinite(bc).all() and (steps >= 1).all() and (steps <= T).all()
    _untouched_past_the_end(kind, acts, steps)
    ok = (twin["margin"] >= C.MARGIN) & ~twin["near"]
    assert np.array_equal(steps[ok], twin["steps"][ok])
    taken = np.arange(T)[None, :] < steps[:, None]
    same = np.where(taken, acts == twin["actions"], True).all(axis=1)
    assert same[ok].all(), np.flatnonzero(ok & ~same)
    assert np.array_equal(fit[ok], twin["fitness"][ok])
    # replay: the twin's physics driven by the device's decisions
    rp = C.episodes(kind, None, T, C.ENV_SEED, C.EPISODE, actions=acts)
    keep = ~rp["near"]
    assert np.array_equal(steps[keep], rp["steps"][keep])
    ef, eb = C.rel_err(fit[keep], rp["fitness"][keep]), C.rel_err(bc[keep], rp["bc"][keep])
    print(f"{label}: replayed fitness error {ef:.3e}, bc error {eb:.3e} (REPLAY_TOL {C.REPLAY_TOL:.0e}); "
          f"{int((~ok).sum())} + {int((~keep).sum())} of {n} members left out")
    assert ef <= C.REPLAY_TOL and eb <= C.REPLAY_TOL, (ef, eb)
    return int((~(ok & keep)).sum())


# ------------------------------------------------------------------ per kind
@pytest.mark.parametrize("T", C.LENGTHS)
@pytest.mark.parametrize("n", C.POPS)
@pytest.mark.parametrize("hidden", C.HIDDEN, ids=lambda h: f"{h[0]}x{h[1]}")
@pytest.mark.parametrize("env_id", DISCRETE)
def test_discrete_kinds(env_id, hidden, n, T):
    """P in {1, 5, 257} (a lone wave, a block with an idle wave, many blocks) x hidden {(1, 1), (3, 7), (64, 64)} x
    T in {1, 2, 40}, with eps null and with eps given: decisions exact, physics replayed within REPLAY_TOL."""
    for with_eps in (False, True):
        kind, _, dev, twin = _case(env_id, hidden, n, T, with_eps)
        left_out = _check_discrete(kind, dev, twin, T, f"{env_id} {hidden} P={n} T={T} eps={with_eps}")
        assert left_out <= 1
        if with_eps and n > 1 and T == 40:
            assert len({a.tobytes() for a in _np(dev["actions"])}) > 1  # the members differ


@needs_ld
@pytest.mark.parametrize("T", C.LENGTHS)
@pytest.mark.parametrize("n", C.POPS)
@pytest.mark.parametrize("hidden", C.HIDDEN, ids=lambda h: f"{h[0]}x{h[1]}")
def test_pendulum(hidden, n, T):
    """Fitness, bc and the f32 torques within PENDULUM_TOL of the long-double restatement, relative to
    max(1, |value|); every episode runs all T steps."""
    for with_eps in (False, True):
        kind, mem, dev, _ = _case("Pendulum-v1", hidden, n, T, with_eps)
        ref = C.episodes_ld(kind, mem, T, C.ENV_SEED, C.EPISODE)
        fit, steps, bc = _np(dev["fitness"]), _np(dev["steps"]), _np(dev["bc"])
        tq = _actions_np(kind, dev["actions"])
        assert (steps == T).all() and np.isfinite(tq).all() and (np.abs(tq) <= 2).all()
        errs = (C.rel_err(fit, ref["fitness"]), C.rel_err(bc, ref["bc"]),
                C.rel_err(tq.astype(np.float64), ref["actions"].astype(np.float64)))
        print(f"Pendulum {hidden} P={n} T={T} eps={with_eps}: fitness {errs[0]:.3e}, bc {errs[1]:.3e}, torque "
              f"{errs[2]:.3e} of PENDULUM_TOL {C.PENDULUM_TOL:.3e}")
        assert max(errs) <= C.PENDULUM_TOL, errs
        if with_eps and n > 1 and T == 40:
            assert len(set(fit.tolist())) == n


@pytest.mark.parametrize("env_id", list(C.KINDS))
def test_nullable_outputs(env_id):
    """steps, bc and actions_out are each optional: the outputs that remain are bitwise the full launch's."""
    kind, hidden, n, T = C.KINDS[env_id], (3, 7), 5, 40
    w, eps, _ = C.case_inputs(kind, hidden, n, True)
    _, _, full, _ = _case(env_id, hidden, n, T, True)
    for outputs in ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1)):
        r = _launch(kind, w, eps, n, hidden, T, outputs=outputs)
        assert torch.equal(r["fitness"], full["fitness"])
        for key in ("steps", "bc", "actions"):
            assert r[key] is None or torch.equal(r[key], full[key]), key


# ------------------------------------------------------------------ early exit, the goal branch
def test_cartpole_terminates_inside_the_limit():
    """Raw randn weights drop the pole: at T = 100 the members' episodes end early (the twin: 9 .. 100 steps,
    median 17), fitness = steps, and actions_out past each member's last step is untouched."""
    kind, hidden, n, T = R.CARTPOLE, (64, 64), 257, 100
    rs = np.random.RandomState(5)
    mem = [[rs.randn(4, 64), rs.randn(64, 64), rs.randn(64, 2)] for _ in range(n)]
    eps = np.stack([C.flat(m) for m in mem])  # w = 0, sigma * eps = the members: eps = theta / sigma
    w = [np.zeros((4, 64)), np.zeros((64, 64)), np.zeros((64, 2))]
    dev = _launch(kind, w, eps / C.SIGMA, n, hidden, T)
    mem = C.members(w, eps / C.SIGMA, C.SIGMA)
    twin = C.episodes(kind, mem, T, C.ENV_SEED, C.EPISODE)
    assert _check_discrete(kind, dev, twin, T, "CartPole raw weights T=100") <= 1
    steps = _np(dev["steps"])
    assert steps.min() < 20 and np.median(steps) < 50 and (steps < T).sum() > n // 2
    assert np.array_equal(_np(dev["fitness"]), steps.astype(np.float64))


@pytest.mark.parametrize("episode", [0, 1, 2, 3])
def test_mountaincar_goal(episode):
    """The constructed policy (push the way the car moves) reaches the goal inside T = 200: steps is the twin's,
    fitness = -steps, bc[0] >= 0.5, actions_out past the last step and all the guards untouched."""
    kind = R.MOUNTAINCAR
    w = C.mountaincar_policy()
    dev = _launch(kind, w, None, 1, (1, 1), 200, episode=episode)
    twin = C.episodes(kind, [w], 200, C.ENV_SEED, episode)
    assert twin["margin"][0] >= C.MARGIN and not twin["near"][0]
    steps, fit, bc = int(dev["steps"][0]), float(dev["fitness"][0]), _np(dev["bc"])[0]
    print(f"MountainCar goal, episode {episode}: {steps} steps, final position {bc[0]:.4f}")
    assert steps == int(twin["steps"][0]) and steps < 200
    assert fit == -steps and bc[0] >= 0.5 and bc[1] >= 0
    acts = _np(dev["actions"])
    _untouched_past_the_end(kind, acts, np.array([steps]))
    assert np.array_equal(acts[0, :steps], twin["actions"][0, :steps])
    assert C.rel_err(bc[None], twin["bc"]) <= C.REPLAY_TOL


# ------------------------------------------------------------------ sharding, determinism, episode
@pytest.mark.parametrize("env_id", list(C.KINDS))
def test_member_slices_and_reruns(env_id):
    """Members [3, 8) evaluated with member0 = 3 on the eps rows 3..7 equal that slice of the [0, 10) call bitwise
    (the action draw is keyed by the global member); two calls with the same arguments are bitwise equal."""
    kind, hidden, T = C.KINDS[env_id], (3, 7), 40
    w, eps, _ = C.case_inputs(kind, hidden, 10, True)
    full = _launch(kind, w, eps, 10, hidden, T)
    again = _launch(kind, w, eps, 10, hidden, T)
    part = _launch(kind, w, eps[3:8], 5, hidden, T, member0=3)
    for key in ("fitness", "steps", "bc", "actions"):
        assert torch.equal(full[key], again[key]), key
        assert torch.equal(part[key], full[key][3:8]), key
    if kind != R.PENDULUM:  # without the offset the same rows draw other actions
        shifted = _launch(kind, w, eps[3:8], 5, hidden, T)
        assert not torch.equal(shifted["actions"], part["actions"])


@pytest.mark.parametrize("env_id", list(C.KINDS))
def test_episode_sets_the_start_state(env_id):
    """A different `episode` starts from the twin's draw for that episode: after one step (T = 1) bc is the
    twin's physics of reset_state(gid 0, episode) under the device's action, and two episodes differ.  The high
    key word matters."""
    kind, hidden = C.KINDS[env_id], (3, 7)
    w, eps, _ = C.case_inputs(kind, hidden, 5, True)
    seen = []
    for episode, seed in ((0, C.ENV_SEED), (7, C.ENV_SEED), (7, C.ENV_SEED & 0xFFFFFFFF)):
        dev = _launch(kind, w, eps, 5, hidden, 1, episode=episode, env_seed=seed)
        s0 = np.repeat(R.reset_state(kind, seed, [0], [episode]), 5, axis=0)
        s1, rew, _, _ = R.physics(kind, s0, _actions_np(kind, dev["actions"])[:, 0])
        assert C.rel_err(_np(dev["bc"]), s1[:, :2]) <= C.REPLAY_TOL
        assert C.rel_err(_np(dev["fitness"]), rew.astype(np.float32).astype(np.float64)) <= C.REPLAY_TOL
        seen.append(_np(dev["bc"]).copy())
    assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[1], seen[2])


# ------------------------------------------------------------------ refusals
BAD = {"kind=-1": dict(kind=-1), "kind=4": dict(kind=4), "w=None": dict(w=None), "fitness=None": dict(fitness=None),
       "P=0": dict(P=0), "P=-1": dict(P=-1), "T=0": dict(T=0), "member0=-1": dict(member0=-1),
       "H1=0": dict(H1=0), "H1=65": dict(H1=65), "H2=0": dict(H2=0), "H2=65": dict(H2=65)}


@pytest.mark.parametrize("bad", list(BAD))
def test_refusals(bad):
    """Unknown kind, null w / fitness, empty P / T, negative member0 and hidden sizes outside [1, 64] raise
    NativeError before anything is launched: every output keeps its pre-fill."""
    native = _native()
    arena = Arena()
    w = torch.zeros(6 * 65 + 65 * 65 + 65 * 3, dtype=F64, device="cuda")
    eps = torch.zeros(4, w.numel(), dtype=F64, device="cuda")
    fit, steps = arena.new(4, F64, init=NAN), arena.new(4, I32)
    bc, acts = arena.new((4, 2), F64, init=NAN), arena.new((4, 5), I32)
    kw = dict(kind=R.ACROBOT, w=w, fitness=fit, P=4, T=5, member0=0, H1=16, H2=12)
    kw.update(BAD[bad])
    with pytest.raises(native.NativeError, match="ppox_es_evaluate_control"):
        native.es_evaluate_control(kw["kind"], kw["w"], eps, 0.1, kw["P"], kw["member0"], kw["H1"], kw["H2"], kw["T"],
                                   1, 0, kw["fitness"], steps, bc, acts)
    assert torch.isnan(fit).all() and torch.isnan(bc).all()
    assert (steps == SENT_I32).all() and (acts == SENT_I32).all()
    arena.check()


# ------------------------------------------------------------------ through the class
def _es(env_id="MountainCar-v0", **kw):
    import evolution_strategies as ES
    np.random.seed(11)
    return ES.EvolutionStrategy(env_id, [8, 8], population_size=24, seed=(3 << 32) | 5, dynamics="real", **kw)


def test_class_evaluates_real_episodes():
    """EvolutionStrategy("MountainCar-v0", [8, 8], population_size=24, dynamics="real"): _get_rewards is the twin's
    fitness on the perturbed members (member0 = 0, episode = the generation), get_behavior_char and evaluate the
    twin's on the weights; no xi table is made and the action space is Discrete(3)."""
    es = _es()
    kind = R.MOUNTAINCAR
    assert es.sizes == [2, 8, 8, 3] and es.T == 200 and es.env.kind == kind and not hasattr(es, "xi")
    assert es.model.action_space == "Discrete" and es.model.num_actions == 3
    es.generation = 2
    pop = es._get_population()
    rewards = es._get_rewards(None, pop)
    mem = C.members(es.weights, _np(pop), es.SIGMA)
    twin = C.episodes(kind, mem, 200, es.env_seed, 2)
    ok = (twin["margin"] >= C.MARGIN) & ~twin["near"]
    assert ok.sum() >= 23
    assert rewards.shape == (24,) and np.array_equal(rewards[ok], twin["fitness"][ok])
    assert np.array_equal(es.ep_len[ok], twin["steps"][ok])
    one = C.episodes(kind, [es.weights], 200, es.env_seed, 2)
    assert one["margin"][0] >= C.MARGIN and not one["near"][0]
    b = es.get_behavior_char(es.weights)
    assert b.shape == (1, 2) and C.rel_err(b, one["bc"]) <= C.REPLAY_TOL
    assert es.evaluate(es.weights) == one["fitness"][0]
    a = es.model.predict(np.array([-0.5, 0.0]))
    assert int(a) in (0, 1, 2)


def test_class_runs_and_logs(monkeypatch):
    """run(3) logs reward, novelty, n_koeff and ep_len, and leaves three (1, 2) behaviours in the archive."""
    import logger
    rows = []
    monkeypatch.setattr(logger.TableWriter, "write", lambda self, kv: rows.append(kv))
    es = _es(episode_len=50)
    es.run(3)
    assert len(rows) == 3
    for row in rows:
        assert {"iteration", "reward", "novelty", "n_koeff", "ep_len", "total_time"} <= set(row)
        assert 1 <= row["ep_len"] <= 50 and -50 <= row["reward"] <= 0
    assert len(es.archive) == 3 and all(b.shape == (1, 2) and np.isfinite(b).all() for b in es.archive)
    assert es.ep_len.shape == (24,)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_es_cartpole_learns(seed):
    """ES-NSRA as shipped (run(), 64 members, hidden (8, 8), sigma 0.1, learning rate 0.2) on CartPole-v1: the
    population's mean fitness over the last 5 of 100 generations is >= 3 x that of generation 0 (DESIGN §10's
    criterion for PPO), inside 10 s of wall time.  Measured (tools/es_control_compare.py,
    profiles/es_control/compare.jsonl): 110.0 -> 500.0, 22.7 -> 499.96, 25.6 -> 500.0 on seeds 0, 1, 2, in 0.87,
    0.66 and 0.69 s; the worst ratio, 4.54 on seed 0, leaves the asserted 3 a 1.5 x margin."""
    import time

    import evolution_strategies as ES
    np.random.seed(seed)
    es = ES.EvolutionStrategy("CartPole-v1", [8, 8], population_size=64, sigma=0.1, learning_rate=0.2, seed=seed,
                              dynamics="real")
    means, inner = [], es._get_rewards

    def recorded(pool, population):
        rewards = inner(pool, population)
        means.append(float(rewards.mean()))
        return rewards
    es._get_rewards = recorded
    t0 = time.perf_counter()
    es.run(100, log_interval=10 ** 9)
    wall = time.perf_counter() - t0
    first, last = means[0], float(np.mean(means[-5:]))
    print(f"ES-NSRA CartPole-v1 seed {seed}: generation 0 mean fitness {first:.1f}, last 5 of 100 {last:.2f} "
          f"({last / first:.2f} x), {wall:.2f} s")
    assert len(means) == 100 and last >= 3 * first and wall < 10.0


def test_class_constructor_refusals():
    """The synthetic constructor still refuses a Discrete id; dynamics="real" takes the ids of env.CONTROL_ENVS
    only, and names them."""
    import evolution_strategies as ES
    with pytest.raises(NotImplementedError, match="Box action spaces"):
        ES.EvolutionStrategy("CartPole-v1", [8, 8], population_size=4)
    with pytest.raises(ValueError, match="CartPole-v1, CartPole-v0, MountainCar-v0, Acrobot-v1, Pendulum-v1"):
        ES.EvolutionStrategy("Hopper-v2", [8, 8], population_size=4, dynamics="real")
    with pytest.raises(ValueError, match="'synthetic' or 'real'"):
        ES.EvolutionStrategy("Hopper-v2", [8, 8], population_size=4, dynamics="mujoco")
    es = ES.EvolutionStrategy("Pendulum-v1", [8, 8], population_size=4, dynamics="real", episode_len=10)
    assert es.sizes == [3, 8, 8, 1] and es.model.action_space == "Box"
