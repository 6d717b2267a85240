"""The numpy twin of the real-dynamics envs (tests/real_env_twin.py) pinned on its own: known
behaviours of the tasks, so the GPU tests (test_real_env_gpu.py) compare the kernels against
something that is itself checked.  CPU only."""
import math

import numpy as np
import pytest

import real_env_twin as T


def test_cartpole_falls_at_step_10():
    """From (0.01, 0, 0.01, 0), pushing right every step, the pole passes 12 degrees at step 10."""
    s = np.array([[0.01, 0.0, 0.01, 0.0]])
    for step in range(1, 11):
        s, r, term, _ = T.physics(T.CARTPOLE, s, [1])
        assert r[0] == 1.0
        assert bool(term[0]) == (step == 10), (step, s)


def test_mountaincar_reachability():
    """Always pushing right never gets out of the valley in 200 steps; pushing with the velocity does,
    in 113..125 steps, from every start in [-0.6, -0.4]."""
    p0 = np.linspace(-0.6, -0.4, 21)
    s = np.stack([p0, np.zeros_like(p0)], axis=-1)
    for _ in range(200):
        s, _, term, _ = T.physics(T.MOUNTAINCAR, s, np.full(21, 2))
        assert not term.any()
    s = np.stack([p0, np.zeros_like(p0)], axis=-1)
    reached = np.zeros(21, int)
    for step in range(1, 201):
        nxt, r, term, _ = T.physics(T.MOUNTAINCAR, s, np.where(s[:, 1] >= 0, 2, 0))
        assert (r == -1.0).all()
        reached[(reached == 0) & term] = step
        s = np.where((reached > 0)[:, None], s, nxt)  # a finished car stays put
    print("MountainCar steps to the goal:", reached.tolist())
    assert ((reached >= 113) & (reached <= 125)).all(), reached


def test_mountaincar_wall_and_clips():
    s, _, _, _ = T.physics(T.MOUNTAINCAR, np.array([[-1.19, -0.07]]), [0])
    assert s[0, 0] == -1.2 and s[0, 1] == 0.0
    s, _, term, _ = T.physics(T.MOUNTAINCAR, np.array([[0.55, 0.0699]]), [2])  # cos(3 p) < 0 there: v grows
    assert s[0, 1] == 0.07 and s[0, 0] == 0.6 and term[0]


def test_cartpole_random_policy_mean_length():
    """2,000 random-policy episodes: mean length in [20, 25] (measured 22.4)."""
    env = T.ControlTwin("CartPole-v1", 100, seed=3)
    rs = np.random.RandomState(0)
    lengths = []
    while len(lengths) < 2000:
        out = env.step(rs.randint(0, 2, size=100))
        fin = out["done_len"][out["done"]]
        assert (out["done_ret"][out["done"]] == fin).all()  # reward 1 per step
        lengths.extend(fin.tolist())
    mean = float(np.mean(lengths[:2000]))
    print("CartPole random-policy mean episode length:", mean)
    assert 20.0 <= mean <= 25.0, mean


def test_pendulum_rest_point_and_clip():
    """(th, thd) = (0, 0) with zero torque stays there at reward 0; torques beyond +-2 act as +-2."""
    s = np.zeros((1, 2))
    for _ in range(5):
        s, r, term, _ = T.physics(T.PENDULUM, s, np.zeros((1, 1), np.float32))
        assert (s == 0).all() and r[0] == 0.0 and not term[0]
    s0 = np.array([[0.3, -0.2]])
    a, ra, _, _ = T.physics(T.PENDULUM, s0, np.array([[2.5]], np.float32))
    b, rb, _, _ = T.physics(T.PENDULUM, s0, np.array([[2.0]], np.float32))
    assert (a == b).all() and ra[0] == rb[0]
    # (the wrap's + pi - pi costs an ulp of pi on the angle)
    assert abs(rb[0] + (0.3 * 0.3 + 0.1 * 0.2 * 0.2 + 0.001 * 2.0 * 2.0)) < 1e-15


def test_acrobot_angles_wrap_into_range():
    x = np.concatenate([np.random.RandomState(1).uniform(-50, 50, 10000), [-math.pi, math.pi, 0.0, 3 * math.pi]])
    w = T.wrap_pi(x)
    assert (w >= -math.pi).all() and (w < math.pi).all()
    assert np.abs(np.sin(w) - np.sin(x)).max() < 1e-13  # the same angle
    env = T.ControlTwin("Acrobot-v1", 32, seed=1)
    rs = np.random.RandomState(2)
    for _ in range(300):
        out = env.step(rs.randint(0, 3, size=32))
        th = out["pre_reset_state"][:, :2]
        assert (th >= -math.pi).all() and (th < math.pi).all()
        assert (np.abs(out["pre_reset_state"][:, 2]) <= 4 * math.pi).all()
        assert (np.abs(out["pre_reset_state"][:, 3]) <= 9 * math.pi).all()
        assert ((out["reward"] == 0) == out["terminated"]).all()


def test_reset_draws_are_sharded_by_global_id():
    for env_id, (kind, *_rest) in T.SPECS.items():
        lo, hi = (np.asarray(b) for b in T.RESET_BOUNDS[kind])
        full = T.reset_state(kind, 11, np.arange(67), np.full(67, 4))
        part = T.reset_state(kind, 11, np.arange(23, 46), np.full(23, 4))
        assert np.array_equal(full[23:46], part)
        assert (full >= lo).all() and (full[:, hi > lo] < hi[hi > lo]).all()
        assert not np.array_equal(full, T.reset_state(kind, 11, np.arange(67), np.full(67, 5)))


def test_time_limit_ends_every_episode():
    for env_id in T.SPECS:
        env = T.ControlTwin(env_id, 9, seed=2, max_len=7)
        for t in range(1, 15):
            out = env.step(T.draw_actions(env_id, 2, env.gids, t))
            assert not out["terminated"].any()  # (no task ends on its own this early)
            assert out["done"].all() == (t % 7 == 0) and out["done"].any() == (t % 7 == 0)
            if t % 7 == 0:
                assert (out["done_len"] == 7).all() and (env.ep_len == 0).all() and (env.episode == t // 7).all()


def test_catch_episodes():
    """Every episode is 11 steps and returns -1 or +1; a paddle that tracks the ball's next column
    catches it every time."""
    env = T.CatchTwin(64, seed=5)
    rs = np.random.RandomState(0)
    returns = []
    for t in range(1, 45):
        out = env.step(rs.randint(0, 3, size=64))
        assert out["done"].all() == (t % 11 == 0) and out["done"].any() == (t % 11 == 0)
        if t % 11 == 0:
            assert (out["done_len"] == 11).all()
            returns.extend(out["done_ret"].tolist())
            assert (out["obs"][:, :3] == 0).all()  # stack zeroed, the new episode's frame last
        else:
            assert (out["reward"] == 0).all()
        frame = out["obs"][:, 3]
        assert ((frame == 0) | (frame == 128) | (frame == 255)).all()
        assert ((frame == 255).sum(axis=(1, 2)) == 49).all()
        assert ((frame != 0).sum(axis=(1, 2)) <= 4 * 49).all()
    assert set(returns) == {-1.0, 1.0}

    env = T.CatchTwin(64, seed=6)
    for t in range(1, 56):
        col, _, dx, pad = env.state.T
        nxt = col + dx
        nxt = np.where(nxt < 0, -nxt, np.where(nxt > 11, 22 - nxt, nxt))
        out = env.step(np.where(nxt < pad, 1, np.where(nxt > pad, 2, 0)))
        if t % 11 == 0:
            assert (out["reward"] == 1.0).all()


def test_gpu_test_runs_stay_clear_of_thresholds():
    """The GPU parity test asserts that no step of its (teacher-forced) twin run comes within 1e-12 of a
    threshold; the free-running twin with the same seed and actions shows the seed is a sound choice."""
    for env_id in T.SPECS:
        env = T.ControlTwin(env_id, T.PARITY_N, seed=T.PARITY_SEED)
        for t in range(1, T.PARITY_T + 1):
            assert not env.step(T.draw_actions(env_id, T.PARITY_SEED, env.gids, t))["near"].any(), (env_id, t)


def test_entry_points_validate_before_any_hip_call():
    import ctypes
    import os

    import native
    if not os.path.exists(native.LIB_PATH):
        pytest.skip("libppox.so not built")
    lib = native.load()
    buf = ctypes.create_string_buffer(64)  # 16-byte-misaligned below: address + 1
    p = ctypes.c_void_p(ctypes.addressof(buf))
    assert lib.ppox_control_env_reset(4, p, p, p, 1, 0, 0, p, p, None) == -1000
    assert b"unknown kind" in lib.ppox_last_error()
    assert lib.ppox_control_env_step(-1, p, p, p, p, 1, 0, 0, 200, p, p, p, p, None, None, None) == -1000
    assert b"unknown kind" in lib.ppox_last_error()
    assert lib.ppox_control_env_step(0, p, p, None, p, 1, 0, 0, 200, p, p, p, p, None, None, None) == -1000
    assert b"null pointer" in lib.ppox_last_error()
    assert lib.ppox_control_env_step(0, p, p, p, p, 0, 0, 0, 200, p, p, p, p, None, None, None) == -1000
    assert lib.ppox_control_env_step(0, p, p, p, p, 1, 0, 0, 0, p, p, p, p, None, None, None) == -1000
    assert b"max_len" in lib.ppox_last_error()
    assert lib.ppox_catch_env_reset(None, p, p, 1, 0, 0, None, None, None) == -1000
    odd = ctypes.c_void_p(ctypes.addressof(buf) | 1)
    assert lib.ppox_catch_env_reset(odd, p, p, 1, 0, 0, None, None, None) == -1000
    assert b"16B aligned" in lib.ppox_last_error()
    assert lib.ppox_catch_env_step(p, odd, p, p, p, 1, 0, 0, p, p, None, None, None, None, None) == -1000
    assert lib.ppox_catch_env_step(p, p, p, p, p, 0, 0, 0, p, p, None, None, None, None, None) == -1000


def test_make_env_real_argument_handling():
    import env as E
    with pytest.raises(ValueError, match="CartPole-v1.*Catch-v0"):
        E.make_env("Hopper-v2", dynamics="real")
    with pytest.raises(ValueError, match="supported ids"):
        E.make_env("BreakoutNoFrameskip-v4", dynamics="real")
    with pytest.raises(ValueError, match="dynamics"):
        E.make_env("CartPole-v1", dynamics="gym")
    with pytest.raises(ValueError, match="supported ids"):
        E.DeviceControlEnv("Hopper-v2", 4)
    assert set(E.REAL_ENVS) == set(T.SPECS) | {"Catch-v0"}
    for env_id, (kind, s_dim, obs_dim, n_actions, max_len) in T.SPECS.items():
        k, s, d, space, ml = E.CONTROL_ENVS[env_id]
        assert (k, s, d, ml) == (kind, s_dim, obs_dim, max_len)
        assert (space.n if n_actions else space.shape) == (n_actions or (1,))
