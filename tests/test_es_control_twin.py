"""CPU checks of tests/es_control_twin.py, the numpy restatement that tests/test_es_control_gpu.py holds
ppox_es_evaluate_control to: its episode is real_env_twin.ControlTwin's driven by the same actions, the decision
rule's edges, the constructed MountainCar policy, that the shape table keeps every draw clear of its thresholds,
and where PENDULUM_TOL comes from."""
import numpy as np
import pytest

import es_control_twin as C
import real_env_twin as R

needs_ld = pytest.mark.skipif(not C.ld_ok(), reason=C.LD_SKIP_REASON)
KIND_IDS = pytest.mark.parametrize("env_id", list(C.KINDS))


def _all_cases(kind, lengths=C.LENGTHS):
    for hidden in C.HIDDEN:
        for n in C.POPS:
            for T in lengths:
                for with_eps in (False, True):
                    yield hidden, n, T, with_eps


@KIND_IDS
def test_episode_is_the_control_twins(env_id):
    """One member at a time against ControlTwin(one env, gid 0, same seed, max_len = T, episode 0) driven by the
    twin's own actions: the state after every step, the rewards and the step that is done, bitwise."""
    kind = C.KINDS[env_id]
    T = 40
    _, _, mem = C.case_inputs(kind, (3, 7), 5, True)
    r = C.episodes(kind, mem, T, C.ENV_SEED, 0, trace=True)
    for m in range(5):
        env = R.ControlTwin(env_id, 1, seed=C.ENV_SEED, max_len=T)
        assert np.array_equal(env.state, R.reset_state(kind, C.ENV_SEED, [0], [0]))
        fit = 0.0
        for t in range(int(r["steps"][m])):
            out = env.step(r["actions"][m:m + 1, t])
            assert np.array_equal(out["pre_reset_state"][0], r["states"][m, t]), (m, t)
            assert out["reward64"][0] == r["rewards"][m, t], (m, t)
            fit += float(out["reward"][0])
            assert bool(out["done"][0]) == (t + 1 == r["steps"][m]), (m, t)
        assert fit == r["fitness"][m]
        assert np.array_equal(r["bc"][m], r["states"][m, r["steps"][m] - 1, :2])
        assert np.isnan(r["states"][m, r["steps"][m]:]).all()


@KIND_IDS
def test_one_step(env_id):
    """T = 1: one observation of the shared start state, one decision, one physics step."""
    kind = C.KINDS[env_id]
    w, eps, mem = C.case_inputs(kind, (3, 7), 5, True)
    r = C.episodes(kind, mem, 1, C.ENV_SEED, C.EPISODE)
    s0 = np.repeat(R.reset_state(kind, C.ENV_SEED, [0], [C.EPISODE]), 5, axis=0)
    s1, rew, _, _ = R.physics(kind, s0, r["actions"][:, 0])
    assert (r["steps"] == 1).all() and r["actions"].shape == (5, 1)
    assert np.array_equal(r["bc"], s1[:, :2])
    assert np.array_equal(r["fitness"], rew.astype(np.float32).astype(np.float64))
    if kind != R.PENDULUM:
        W0, W1, W2 = C._stack(mem, np.float64)
        z = C.logits(R.observe(kind, s0).astype(np.float64), W0, W1, W2)
        for m in range(5):  # the matrix products, to rounding: the twin's orders are only orders
            ref = np.arctan(np.arctan(R.observe(kind, s0)[m].astype(np.float64) @ mem[m][0]) @ mem[m][1]) @ mem[m][2]
            np.testing.assert_allclose(z[m], ref, rtol=1e-13, atol=1e-13)


def test_inverse_cdf_edges():
    """The first j < A-1 with u < q_0 + .. + q_j, else A-1: all mass on the last action is the fallback for every
    u (u = 0 too), all mass on the first is action 0, equal logits split [0, 1) in thirds, and the margin is the
    distance to the nearest of the A-1 thresholds."""
    u = np.array([0.0, 0.2, 1.0 / 3.0, 0.5, 0.7, 1.0 - 2.0 ** -24])
    n = len(u)
    a, _ = C.decide(np.tile([-800.0, -800.0, 0.0], (n, 1)), u)
    assert (a == 2).all()
    a, _ = C.decide(np.tile([0.0, -800.0, -800.0], (n, 1)), u)
    assert (a == 0).all()
    a, margin = C.decide(np.zeros((n, 3)), u)
    q = 1.0 / 3.0
    assert a.tolist() == [0, 0, 1, 1, 2, 2]  # u = 1/3 is not below q_0 = 1/3
    np.testing.assert_allclose(margin, np.minimum(np.abs(u - q), np.abs(u - (q + q))), rtol=0, atol=1e-16)
    a, margin = C.decide(np.zeros((n, 2)), u)
    assert a.tolist() == [0, 0, 0, 1, 1, 1] and margin[3] == 0.0
    # the draw is keyed by (step, global member, episode): a slice of the members is that slice of the draw
    full = C.action_uniform(C.ENV_SEED, 5, np.arange(10), 2)
    assert np.array_equal(C.action_uniform(C.ENV_SEED, 5, 3 + np.arange(5), 2), full[3:8])
    assert not np.array_equal(C.action_uniform(C.ENV_SEED, 5, np.arange(10), 3), full)
    assert ((full >= 0) & (full < 1)).all()


@pytest.mark.parametrize("episode", [0, 1, 2, 3])
def test_constructed_mountaincar_policy_reaches_the_goal(episode):
    """Pushing the way the car moves swings it out of the valley: the twin reaches p >= 0.5 inside the 200-step
    limit (172, 93, 92, 123 steps for episodes 0-3 under ENV_SEED, margins >= 3.5e-3), fitness = -steps."""
    r = C.episodes(R.MOUNTAINCAR, [C.mountaincar_policy()], 200, C.ENV_SEED, episode)
    steps = int(r["steps"][0])
    print(f"MountainCar constructed policy, episode {episode}: {steps} steps, margin {r['margin'][0]:.3e}")
    assert 80 <= steps < 200 and r["fitness"][0] == -steps
    assert r["bc"][0, 0] >= 0.5 and r["bc"][0, 1] >= 0
    assert r["margin"][0] >= 1e-6 and not r["near"][0]
    assert (r["actions"][0, :steps] != C.ACTION_FILL).all() and (r["actions"][0, steps:] == C.ACTION_FILL).all()
    idle = C.episodes(R.MOUNTAINCAR, [[np.zeros((2, 1)), np.zeros((1, 1)), np.array([[-800.0, 0.0, -800.0]])]],
                      200, C.ENV_SEED, episode)  # never pushing stays in the valley
    assert idle["steps"][0] == 200 and idle["fitness"][0] == -200.0 and idle["bc"][0, 0] < 0.5


def test_raw_cartpole_weights_terminate_early():
    """Un-scaled randn weights drop the pole: at T = 100 most of 257 members end inside the limit."""
    rs = np.random.RandomState(5)
    mem = [[rs.randn(4, 64), rs.randn(64, 64), rs.randn(64, 2)] for _ in range(257)]
    r = C.episodes(R.CARTPOLE, mem, 100, C.ENV_SEED, C.EPISODE)
    print("CartPole raw weights: steps", r["steps"].min(), np.median(r["steps"]), r["steps"].max())
    assert r["steps"].min() < 20 and np.median(r["steps"]) < 50
    assert np.array_equal(r["fitness"], r["steps"].astype(np.float64))
    assert r["margin"].min() >= C.MARGIN and not r["near"].any()


@KIND_IDS
def test_shape_table_is_clear_of_every_threshold(env_id):
    """Over the whole table of the GPU test (P x hidden x T x eps) the twin alone leaves no member out: every
    draw is at least MARGIN from its thresholds and no physics flag is within real_env_twin.EPS of flipping."""
    kind = C.KINDS[env_id]
    worst = np.inf
    for hidden, n, T, with_eps in _all_cases(kind):
        _, _, mem = C.case_inputs(kind, hidden, n, with_eps)
        r = C.episodes(kind, mem, T, C.ENV_SEED, C.EPISODE)
        assert not r["near"].any(), (hidden, n, T, with_eps)
        worst = min(worst, float(r["margin"].min()))
        assert (r["steps"] >= 1).all() and (r["steps"] <= T).all()
    print(f"{env_id}: smallest margin over the table {worst:.3e}")
    assert worst >= 100 * C.MARGIN


@needs_ld
def test_pendulum_tol_is_16x_the_twins_own_error():
    """PENDULUM_TOL >= 16 x the float64 twin's worst distance from episodes_ld over the Pendulum cases at T = 40,
    and swapping two weights moves the fitness by >= 100 x PENDULUM_TOL in every shape (the first two entries of W1;
    at (1, 1), where W1 has one entry, the first two of W0): the bound cannot hide an index error."""
    kind = R.PENDULUM
    worst = 0.0
    for hidden, n, T, with_eps in _all_cases(kind, lengths=(40,)):
        _, _, mem = C.case_inputs(kind, hidden, n, with_eps)
        r = C.episodes(kind, mem, T, C.ENV_SEED, C.EPISODE)
        l = C.episodes_ld(kind, mem, T, C.ENV_SEED, C.EPISODE)
        worst = max(worst, C.rel_err(r["fitness"], l["fitness"]), C.rel_err(r["bc"], l["bc"]),
                    C.rel_err(r["actions"].astype(np.float64), l["actions"].astype(np.float64)))
    print(f"Pendulum twin vs long double, worst over the table: {worst:.4e}")
    assert C.PENDULUM_TOL == 16 * C.PENDULUM_TWIN_WORST
    assert worst <= C.PENDULUM_TWIN_WORST
    for hidden in C.HIDDEN:
        w = C.case_weights(kind, hidden)
        base = C.episodes(kind, [w], 40, C.ENV_SEED, C.EPISODE)["fitness"][0]
        sw = [x.copy() for x in w]
        tgt = sw[1].reshape(-1) if sw[1].size >= 2 else sw[0].reshape(-1)
        tgt[0], tgt[1] = tgt[1], tgt[0]
        moved = abs(C.episodes(kind, [sw], 40, C.ENV_SEED, C.EPISODE)["fitness"][0] - base) / max(1.0, abs(base))
        print(f"Pendulum {hidden}: a swapped weight pair moves the fitness by {moved:.3e}")
        assert moved >= 100 * C.PENDULUM_TOL, (hidden, moved)


@needs_ld
def test_acrobot_replay_long_double():
    """The float64 twin's Acrobot episodes, replayed in long double on the same actions, end at the same step and
    within 1e-13 of the same state: the replayed physics is well conditioned at T <= 40, so REPLAY_TOL = 1e-12
    holds the kernel to rounding, not to luck."""
    kind = R.ACROBOT
    worst = 0.0
    for hidden, n, T, with_eps in _all_cases(kind, lengths=(40,)):
        _, _, mem = C.case_inputs(kind, hidden, n, with_eps)
        r = C.episodes(kind, mem, T, C.ENV_SEED, C.EPISODE)
        l = C.episodes_ld(kind, None, T, C.ENV_SEED, C.EPISODE, actions=r["actions"])
        assert np.array_equal(l["steps"], r["steps"])
        worst = max(worst, C.rel_err(r["fitness"], l["fitness"]), C.rel_err(r["bc"], l["bc"]))
    print(f"Acrobot twin replay vs long double, worst over the table: {worst:.4e}")
    assert worst <= 1e-13


def test_replay_reproduces_the_free_run():
    """episodes(actions=...) on the twin's own actions is the twin's own episode, bitwise (Discrete and Pendulum)."""
    for kind in (R.CARTPOLE, R.PENDULUM):
        _, _, mem = C.case_inputs(kind, (3, 7), 5, True)
        r = C.episodes(kind, mem, 40, C.ENV_SEED, C.EPISODE)
        p = C.episodes(kind, None, 40, C.ENV_SEED, C.EPISODE, actions=r["actions"])
        for k in ("fitness", "steps", "bc"):
            assert np.array_equal(r[k], p[k]), k
