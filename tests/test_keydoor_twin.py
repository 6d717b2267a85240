"""The numpy twin of KeyDoor-v0 (tests/keydoor_twin.py) pinned on its own, the library's host-side
layout function and argument checks, and make_env's handling of the id: so the GPU tests
(test_keydoor_gpu.py) compare the kernels against something that is itself checked.  CPU only."""
import ctypes
import os

import numpy as np
import pytest

import keydoor_twin as K


def _lib():
    import native
    if not os.path.exists(native.LIB_PATH):
        pytest.skip("libppox.so not built")
    return native.load()


def test_layout_matches_the_library():
    """ppox_keydoor_layout (host only) == the twin's layout for 64 seeds (a 64-bit one among them); the key lies
    in the left room, the goal in the right room, the door row in 1..10."""
    import native
    _lib()
    for seed in list(range(63)) + [0x9E3779B97F4A7C15]:
        lay = K.layout(seed)
        assert native.keydoor_layout(seed) == lay, seed
        assert 1 <= lay["door_row"] <= 10
        assert 1 <= lay["key"][0] <= 10 and 1 <= lay["key"][1] <= 5
        assert 1 <= lay["goal"][0] <= 10 and 7 <= lay["goal"][1] <= 10
        walls = K.wall_mask(lay)
        assert not walls[lay["key"]] and not walls[lay["goal"]] and not walls[lay["door_row"], K.DIVIDER]
        assert walls.sum() == 44 + 10 - 1
    assert len({tuple(sorted(K.layout(s).items())) for s in range(63)}) > 50  # the seed matters


def test_entry_points_validate_before_any_hip_call():
    lib = _lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.c_void_p(ctypes.addressof(buf))
    odd = ctypes.c_void_p(ctypes.addressof(buf) | 1)
    err = lib.ppox_last_error
    assert lib.ppox_keydoor_layout(0, None) == -1000
    assert b"null pointer" in err()
    # reset: obs, state, episode, visits, N, env_offset, seed, ep_ret, ep_len, stream
    assert lib.ppox_keydoor_env_reset(None, p, p, p, 1, 0, 0, None, None, None) == -1000
    assert b"null pointer" in err()
    assert lib.ppox_keydoor_env_reset(p, p, p, None, 1, 0, 0, None, None, None) == -1000
    assert b"null pointer" in err()
    assert lib.ppox_keydoor_env_reset(p, p, p, p, 0, 0, 0, None, None, None) == -1000
    assert b"must be positive" in err()
    assert lib.ppox_keydoor_env_reset(p, p, p, p, 1, -1, 0, None, None, None) == -1000
    assert b"non-negative" in err()
    assert lib.ppox_keydoor_env_reset(p, p, p, p, 1, 0xFFFFFFFE, 0, None, None, None) == -1000
    assert b"0xFFFFFFFF" in err()
    assert lib.ppox_keydoor_env_reset(p, p, p, p, 0xFFFFFFFF, 0, 0, None, None, None) == -1000
    assert b"0xFFFFFFFF" in err()
    assert lib.ppox_keydoor_env_reset(odd, p, p, p, 1, 0, 0, None, None, None) == -1000
    assert b"16B aligned" in err()
    assert lib.ppox_keydoor_env_reset(p, p, p, p, 1, 0, 0, p, None, None) == -1000
    assert b"pair" in err()
    # step: obs_in, obs_out, actions, state, episode, visits, N, env_offset, seed, max_len, rewards, dones,
    #       ep_ret, ep_len, done_ret, done_len, stream
    tail = (None, None, None, None, None)
    assert lib.ppox_keydoor_env_step(p, p, None, p, p, p, 1, 0, 0, 200, p, p, *tail) == -1000
    assert b"null pointer" in err()
    assert lib.ppox_keydoor_env_step(p, p, p, p, p, None, 1, 0, 0, 200, p, p, *tail) == -1000
    assert b"null pointer" in err()
    assert lib.ppox_keydoor_env_step(p, p, p, p, p, p, 0, 0, 0, 200, p, p, *tail) == -1000
    assert b"must be positive" in err()
    assert lib.ppox_keydoor_env_step(p, p, p, p, p, p, 2, 0xFFFFFFFD, 0, 200, p, p, *tail) == -1000
    assert b"0xFFFFFFFF" in err()
    assert lib.ppox_keydoor_env_step(p, p, p, p, p, p, 1, 0, 0, 0, p, p, *tail) == -1000
    assert b"max_len" in err()
    assert lib.ppox_keydoor_env_step(odd, p, p, p, p, p, 1, 0, 0, 200, p, p, *tail) == -1000
    assert b"16B aligned" in err()
    assert lib.ppox_keydoor_env_step(p, odd, p, p, p, p, 1, 0, 0, 200, p, p, *tail) == -1000
    assert b"16B aligned" in err()
    assert lib.ppox_keydoor_env_step(p, p, p, p, p, p, 1, 0, 0, 200, p, p, None, p, None, None, None) == -1000
    assert b"pair" in err()


def test_make_env_argument_handling():
    import env as E
    import real_env_twin as T
    assert E.GRID_ENVS == ("KeyDoor-v0",)
    assert set(E.REAL_ENVS) == set(T.SPECS) | {"Catch-v0"}  # unchanged
    with pytest.raises(ValueError, match="CartPole-v1.*Catch-v0.*KeyDoor-v0"):
        E.make_env("Hopper-v2", dynamics="real")
    with pytest.raises(ValueError, match="dynamics"):
        E.make_env("KeyDoor-v0", dynamics="gym")
    assert issubclass(E.DeviceKeyDoorEnv, E.DeviceAtariEnv)
    assert not E.is_atari("KeyDoor-v0")  # dynamics="synthetic" keeps treating the id as a vector env


def test_bfs_policy_reaches_the_goal_from_every_start():
    """From each of the 50 start cells, on 8 layouts, the shortest-path policy is at the goal within 40 steps,
    in exactly the distance the search reports, holding the key."""
    for seed in range(8):
        lay = K.layout(seed)
        policy, dist = K.bfs_policy(lay)
        starts = np.array([[r, c, int((r, c) == lay["key"]), 0] for r in range(1, 11) for c in range(1, 6)], np.int32)
        s, steps = starts.copy(), np.zeros(50, int)
        arrived = np.zeros(50, bool)
        for t in range(1, 41):
            nxt, rew, reached, ev = K.physics(s, policy[s[:, 2], s[:, 0], s[:, 1]], lay)
            assert not (ev["wall_bumps"] | ev["refused_doors"])[~arrived].any()
            steps[reached & ~arrived] = t
            s = np.where(arrived[:, None], s, nxt)  # an env that arrived stays put
            arrived |= reached
        assert arrived.all() and (s[:, 2] == 1).all(), seed
        assert np.array_equal(steps, dist[starts[:, 2], starts[:, 0], starts[:, 1]])
        assert 0 < steps.max() <= 40


def test_door_refuses_without_the_key_and_admits_with_it():
    lay = K.layout(0)
    d = lay["door_row"]
    for has, col_after in ((0, 5), (1, 6)):
        s = np.array([[d, 5, has, 0]], np.int32)
        nxt, rew, reached, ev = K.physics(s, [4], lay)
        assert tuple(nxt[0]) == (d, col_after, has, 0) and rew[0] == 0.0
        assert bool(ev["refused_doors"][0]) == (has == 0) and bool(ev["door_passages"][0]) == (has == 1)
        assert not ev["wall_bumps"][0]
    # the rest of column 6 is wall either way, as is the border; an unknown action is stay
    other = d + 1 if d < 10 else d - 1
    for has in (0, 1):
        nxt, _, _, ev = K.physics(np.array([[other, 5, has, 0]], np.int32), [4], lay)
        assert tuple(nxt[0, :2]) == (other, 5) and ev["wall_bumps"][0]
    nxt, _, _, ev = K.physics(np.array([[1, 1, 0, 0]] * 4, np.int32), [1, 3, 7, -2], lay)
    assert (nxt[:, :2] == 1).all() and ev["wall_bumps"].tolist() == [True, True, False, False]
    # stepping on the key picks it up, and the single frame shows it: door and key cells go dark
    kr, kc = lay["key"]
    s = np.array([[kr, kc - 1 if kc > 1 else kc + 1, 0, 0]], np.int32)
    nxt, _, _, ev = K.physics(s, [4 if kc > 1 else 3], lay)
    assert tuple(nxt[0]) == (kr, kc, 1, 0) and ev["key_pickups"][0]
    before, after = K.cells(s, lay)[0], K.cells(nxt, lay)[0]
    assert before[kr, kc] == K.KEY and before[d, 6] == K.DOOR and after[kr, kc] == K.AGENT and after[d, 6] == K.FLOOR
    assert before[lay["goal"]] == K.GOAL and before[0, 0] == K.WALL and (K.frame(s, lay)[0, ::7, ::7] == before).all()
    # the goal pays 1 and nothing else does
    gr, gc = lay["goal"]
    nxt, rew, reached, _ = K.physics(np.array([[gr, gc - 1 if gc > 7 else gc + 1, 1, 0]], np.int32),
                                     [4 if gc > 7 else 3], lay)
    assert reached[0] and rew[0] == 1.0


def test_time_limit_ends_every_episode():
    """max_len = 7: every env is done at its 7th step (no goal is that near a start: the door is in the way)."""
    env = K.KeyDoorTwin(9, seed=2, max_len=7, render=False)
    for t in range(1, 15):
        out = env.step(K.draw_actions(2, env.gids, t))
        assert not out["reached"].any()
        assert out["done"].all() == (t % 7 == 0) and out["done"].any() == (t % 7 == 0)
        if t % 7 == 0:
            assert (out["done_len"] == 7).all() and (env.ep_len == 0).all() and (env.episode == t // 7).all()
            assert (out["done_ret"] == 0).all()


def test_slices_reproduce_the_whole_and_visits_count_every_entry():
    """Envs [0, 67) == the same envs as three twins at env_offset 0 / 23 / 46; the visits tables add up, and
    each total is steps + resets: every state entered is counted once."""
    seed, steps = K.PARITY_SEED, 48
    policy, _ = K.bfs_policy(K.layout(seed))
    whole = K.KeyDoorTwin(67, seed=seed, max_len=K.PARITY_MAX_LEN)
    parts = [K.KeyDoorTwin(n, seed=seed, env_offset=off, max_len=K.PARITY_MAX_LEN)
             for n, off in ((23, 0), (23, 23), (21, 46))]
    assert np.array_equal(whole.obs, np.concatenate([p.obs for p in parts]))
    n_done = 0
    for t in range(1, steps + 1):
        out = whole.step(K.draw_actions(seed, whole.gids, t, whole.state, policy))
        outs = [p.step(K.draw_actions(seed, p.gids, t, p.state, policy)) for p in parts]
        for k in ("obs", "reward", "done"):
            assert np.array_equal(out[k], np.concatenate([o[k] for o in outs])), (t, k)
        n_done += int(out["done"].sum())
    assert n_done > 67
    assert np.array_equal(whole.visits, sum(p.visits for p in parts))
    assert whole.visits.sum() == 67 * steps + 67 + n_done
    assert whole.visits[:, K.wall_mask(whole.layout)].sum() == 0  # nobody stands in a wall
    assert whole.visits[0, :, 7:].sum() == 0                     # or beyond the door without the key


def test_gpu_parity_run_covers_every_branch():
    """The twin's own run at the GPU parity test's shape (N = 67, T = 64, max_len = 40, the mixed action stream,
    PARITY_SEED) takes every branch of the step at least three times."""
    seed = K.PARITY_SEED
    policy, _ = K.bfs_policy(K.layout(seed))
    env = K.KeyDoorTwin(K.PARITY_N, seed=seed, max_len=K.PARITY_MAX_LEN, render=False)
    for t in range(1, K.PARITY_T + 1):
        env.step(K.draw_actions(seed, env.gids, t, env.state, policy))
    print("KeyDoor parity run events:", env.counts)
    assert set(env.counts) == set(K.EVENTS)
    for name, count in env.counts.items():
        assert count >= 3, (name, env.counts)


@pytest.mark.parametrize("seed", K.GPU_TEST_SEEDS)
def test_random_policy_rarely_reaches_the_goal(seed):
    """What makes the task sparse: at max_len = 200 a uniform random policy reaches the goal in fewer than 10 %
    of at least 2,000 episodes, for each seed the GPU tests use (DESIGN.md §11 holds the measured values)."""
    rate, episodes = K.random_policy_rate(seed, max_len=200, n_envs=256, steps=2000)
    print(f"KeyDoor seed {seed}: random-policy goal rate {100 * rate:.2f} % over {episodes} episodes")
    assert episodes >= 2000
    assert rate < 0.10
