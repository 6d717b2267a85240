"""The real-dynamics device envs (csrc/env_real.hip: classic control, Catch) against their numpy
twin (tests/real_env_twin.py), through the public classes and the algorithm constructors."""
import os
import time

import numpy as np
import pytest
import torch

import real_env_twin as T

pytestmark = pytest.mark.gpu

N_ENVS, T_STEPS, SEED = T.PARITY_N, T.PARITY_T, T.PARITY_SEED
F32_ULP2 = 2.4e-7  # two f32 ulps at 1: the cos / sin observation components
LEARN_ITERS = 12   # iterations of 64 envs x 128 steps in test_cartpole_learns


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _step_buffers(n):
    return dict(rewards=torch.empty(n, device="cuda"), dones=torch.empty(n, dtype=torch.uint8, device="cuda"),
                done_ret=torch.empty(n, device="cuda"), done_len=torch.empty(n, dtype=torch.int32, device="cuda"))


def _ulps_f32(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia, ib = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia), np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    return np.abs(ia - ib)


def _teacher_forced(env_id, max_len, steps):
    """Each step: download the device env's state and bookkeeping, step the twin from exactly there with the
    same actions, compare everything the step wrote (a free run would drift, then hide faults)."""
    import env as E
    kind, s_dim, obs_dim, n_actions, _ = T.SPECS[env_id]
    n = N_ENVS
    dev = E.DeviceControlEnv(env_id, n, seed=SEED, max_len=max_len)
    twin = T.ControlTwin(env_id, n, seed=SEED, max_len=max_len)
    obs = torch.full((n, obs_dim), float("nan"), device="cuda")
    dev.reset_into(obs)
    assert dev.state.dtype == torch.float64 and dev.state.shape == (n, s_dim) and dev.episode.dtype == torch.int32
    # reset: bit for bit the twin's Philox draw
    assert np.array_equal(dev.state.cpu().numpy(), twin.state)
    assert (dev.episode == 0).all() and (dev.ep_len == 0).all() and (dev.ep_ret == 0).all()
    exact_obs = kind in (T.CARTPOLE, T.MOUNTAINCAR)
    b = _step_buffers(n)
    worst = dict(state=0.0, obs=0.0, reward=0.0)
    n_resets = n_near = 0
    for t in range(1, steps + 1):
        twin.state = dev.state.cpu().numpy()
        twin.episode = dev.episode.cpu().numpy()
        twin.ep_ret, twin.ep_len = dev.ep_ret.cpu().numpy(), dev.ep_len.cpu().numpy()
        prev_ret = twin.ep_ret.copy()
        a = T.draw_actions(env_id, SEED, twin.gids, t)
        dev.step_into(obs, obs, _dev(a), b["rewards"], b["dones"], b["done_ret"], b["done_len"])
        exp = twin.step(a)
        n_near += int(exp["near"].sum())
        got_state, got_obs = dev.state.cpu().numpy(), obs.cpu().numpy()
        rew, done = b["rewards"].cpu().numpy(), b["dones"].cpu().numpy().astype(bool)
        # flags first: with them equal, the same envs were reset on both sides
        assert np.array_equal(done, exp["done"]), (env_id, t)
        assert np.array_equal(dev.episode.cpu().numpy(), twin.episode)
        assert np.array_equal(dev.ep_len.cpu().numpy(), twin.ep_len)
        assert np.array_equal(b["done_len"].cpu().numpy(), exp["done_len"])
        # a reset env holds the twin's draw for (global id, new episode index) bit for bit
        assert np.array_equal(got_state[done], twin.state[done])
        n_resets += int(done.sum())
        err = np.abs(got_state - twin.state) / np.maximum(1.0, np.abs(twin.state))
        worst["state"] = max(worst["state"], float(err.max()))
        assert err.max() <= 1e-12, (env_id, t, err.max())
        if exact_obs:
            assert np.array_equal(got_obs, got_state.astype(np.float32))
        else:
            # against the device's own state: the f64 -> f32 cast of the velocities is exact, cos / sin within 2 ulps
            ref = T.observe(kind, got_state)
            trig = slice(0, 4) if kind == T.ACROBOT else slice(0, 2)
            oerr = np.abs(got_obs[:, trig].astype(np.float64) - ref[:, trig])
            worst["obs"] = max(worst["obs"], float(oerr.max()))
            assert oerr.max() <= F32_ULP2
            assert np.array_equal(got_obs[:, trig.stop:], ref[:, trig.stop:])
        if kind == T.PENDULUM:
            # f32 casts of two f64 costs that agree to 1e-12 relative: at most one f32 ulp apart
            ulps = _ulps_f32(rew, exp["reward"])
            worst["reward"] = max(worst["reward"], float(ulps.max()))
            assert ulps.max() <= 1
            # the bookkeeping is exact given the device's own reward
            ret = (prev_ret + rew).astype(np.float32)
        else:
            assert np.array_equal(rew, exp["reward"])
            ret = (prev_ret + exp["reward"]).astype(np.float32)
        assert np.array_equal(dev.ep_ret.cpu().numpy(), np.where(done, np.float32(0), ret))
        assert np.array_equal(b["done_ret"].cpu().numpy(), np.where(done, ret, np.float32(np.nan)), equal_nan=True)
    print(f"{env_id} max_len={max_len}: worst state err {worst['state']:.3e} (bound 1e-12), cos/sin obs err "
          f"{worst['obs']:.3e} (bound {F32_ULP2}), reward ulps {worst['reward']:.0f}; {n_resets} auto-resets, "
          f"{n_near} near-threshold steps")
    # a flag may differ only when a threshold quantity is within 1e-12 of its threshold: the cap is zero such steps
    assert n_near == 0
    return n_resets


@pytest.mark.parametrize("env_id", list(T.SPECS))
def test_step_matches_twin_teacher_forced(env_id):
    resets = _teacher_forced(env_id, None, T_STEPS)
    if env_id.startswith("CartPole"):
        assert resets > N_ENVS  # random play drops the pole in ~22 steps: the auto-reset path ran


@pytest.mark.parametrize("env_id", list(T.SPECS))
def test_time_limit(env_id):
    """max_len = 7: every env reports done at its 7th step with done_len == 7 (and again at the 14th)."""
    import env as E
    assert _teacher_forced(env_id, 7, 15) == 2 * N_ENVS
    dev = E.DeviceControlEnv(env_id, N_ENVS, seed=SEED, max_len=7)
    obs = dev.reset()
    for t in range(1, 8):
        a = _dev(T.draw_actions(env_id, SEED, np.arange(N_ENVS), t))
        obs, rew, done, infos = dev.step(a)
        assert bool(done.all()) == (t == 7) and bool(done.any()) == (t == 7)
    assert all(i["episode"]["l"] == 7 for i in infos)
    assert (dev.episode == 1).all()


def _sharded_run(env_id, sizes, steps, seed):
    """The envs [0, sum(sizes)) as len(sizes) env objects at consecutive offsets: per object the list over
    steps of (obs, rewards, dones)."""
    import env as E
    outs, off = [], 0
    for n in sizes:
        if env_id == "Catch-v0":
            dev = E.DeviceCatchEnv(env_id, n, seed=seed, env_offset=off)
        else:
            dev = E.DeviceControlEnv(env_id, n, seed=seed, env_offset=off)
        gids = np.arange(off, off + n)
        obs = dev.reset()
        rows = [(obs.clone(), None, None)]
        for t in range(1, steps + 1):
            obs, rew, done, _ = dev.step(_dev(T.draw_actions(env_id, seed, gids, t)))
            rows.append((obs.clone(), rew.clone(), done.clone()))
        outs.append(rows)
        off += n
    return outs


@pytest.mark.parametrize("env_id", ["CartPole-v1", "Catch-v0"])
def test_sharding_never_changes_the_data(env_id):
    """Envs [0, 67) as one object == the same envs as three objects at env_offset 0 / 23 / 46, bit for bit."""
    (whole,), parts = _sharded_run(env_id, [67], 40, 9), _sharded_run(env_id, [23, 23, 21], 40, 9)
    n_done = 0
    for t in range(41):
        for k in range(3):
            if whole[t][k] is None:
                continue
            assert torch.equal(whole[t][k], torch.cat([p[t][k] for p in parts])), (t, k)
        n_done += 0 if whole[t][2] is None else int(whole[t][2].sum())
    assert n_done >= 67  # episodes ended and restarted on the way


def test_catch_frames_match_twin():
    """N = 5, 34 steps (three full episodes and an auto-reset boundary): frames, rewards, dones and state
    bit-exact; on done the stack is zeroed and the new episode's frame is last."""
    import env as E
    n, seed = 5, 4
    dev, twin = E.DeviceCatchEnv("Catch-v0", n, seed=seed, env_offset=3), T.CatchTwin(n, seed=seed, env_offset=3)
    assert dev.action_space.n == 3 and dev.observation_space.shape == (4, 84, 84) and dev.obs_dtype == torch.uint8
    obs = torch.full((n, 4, 84, 84), 77, dtype=torch.uint8, device="cuda")
    dev.reset_into(obs)
    assert np.array_equal(obs.cpu().numpy(), twin.obs)
    assert np.array_equal(dev.state.cpu().numpy(), twin.state)
    nxt = torch.full_like(obs, 77)
    b = _step_buffers(n)
    for t in range(1, 35):
        a = T.draw_actions("Catch-v0", seed, twin.gids, t)
        dev.step_into(obs, nxt, _dev(a), b["rewards"], b["dones"], b["done_ret"], b["done_len"])
        exp = twin.step(a)
        got = nxt.cpu().numpy()
        assert np.array_equal(got, exp["obs"]), t
        assert np.array_equal(b["rewards"].cpu().numpy(), exp["reward"])
        assert np.array_equal(b["dones"].cpu().numpy().astype(bool), exp["done"])
        assert exp["done"].all() == (t % 11 == 0) and exp["done"].any() == (t % 11 == 0)
        assert np.array_equal(b["done_ret"].cpu().numpy(), exp["done_ret"], equal_nan=True)
        assert np.array_equal(b["done_len"].cpu().numpy(), exp["done_len"])
        assert np.array_equal(dev.state.cpu().numpy(), twin.state)
        assert np.array_equal(dev.episode.cpu().numpy(), twin.episode)
        assert np.array_equal(dev.ep_ret.cpu().numpy(), twin.ep_ret)
        assert np.array_equal(dev.ep_len.cpu().numpy(), twin.ep_len)
        if t % 11 == 0:
            assert (got[:, :3] == 0).all() and (got[:, 3] == T.catch_frame(twin.state)).all()
        obs, nxt = nxt, obs
    assert (dev.episode == 3).all()


def _same_bits(u, v):
    """torch.equal on the bit patterns (done_ret holds NaNs where no episode ended)."""
    if u.dtype == torch.float32:
        u, v = u.view(torch.int32), v.view(torch.int32)
    return torch.equal(u, v)


def _quiet(algo, env_id):
    import logger
    logger.configure(algo, env_id, quiet=True)


def test_catch_collect_graph_matches_eager():
    """The captured collect loop accepts the Catch env (a DeviceAtariEnv): two collects replayed from the
    graph == two eager ones (PPOX_COLLECT_GRAPH=0) in a fresh object with the same seed, bit for bit."""
    import ppo
    _quiet("PPO", "Catch-v0")

    def run(graph):
        os.environ["PPOX_COLLECT_GRAPH"] = "1" if graph else "0"
        try:
            np.random.seed(0)
            torch.manual_seed(0)
            alg = ppo.PPO(env_id="Catch-v0", dynamics="real", n_envs=8, nstep=16, batch_size=64, n_epochs=1,
                          quiet=True, seed=3)
        finally:
            del os.environ["PPOX_COLLECT_GRAPH"]
        outs = []
        for _ in range(2):
            alg.collect_samples()
            ro = alg.rollout
            outs.append([x.clone() for x in (ro.actions, ro.rewards, ro.values, ro.log_probs, ro.masks, ro.obs_slots,
                                             ro.done_ret, ro.done_len, alg.env.state, alg.env.episode)])
        return alg, outs

    (ea, a), (ga, g) = run(False), run(True)
    assert type(ga.env).__name__ == "DeviceCatchEnv" and ga._collect_graph_ok() and not ea._collect_graph_ok()
    assert ea._cgraph is None and ga._cgraph is not None
    for xa, xg in zip(a, g):
        for u, v in zip(xa, xg):
            assert _same_bits(u, v)
    masks = torch.cat([g[0][4], g[1][4]])  # 32 steps: the 11th and 22nd end every episode
    assert masks[10].all() and masks[21].all() and int(masks.sum()) == 16
    assert set(torch.cat([g[0][1], g[1][1]])[masks.bool()].tolist()) <= {-1.0, 1.0}


def test_box_actions_reach_the_env():
    """Pendulum under PPO: the rollout's rewards are the twin's for the rollout's own stored actions."""
    import env as E
    import ppo
    _quiet("PPO", "Pendulum-v1")
    n, nstep, seed = 8, 8, 6
    np.random.seed(0)
    torch.manual_seed(0)
    env = E.make_env("Pendulum-v1", n_envs=n, seed=seed, dynamics="real", normalize=False)
    assert isinstance(env, E.DeviceControlEnv)
    alg = ppo.PPO(env_id="Pendulum-v1", dynamics="real", n_envs=n, nstep=nstep, batch_size=32, n_epochs=1, quiet=True,
                  seed=seed, env=env)
    alg.collect_samples()
    ro = alg.rollout
    acts, rews = ro.actions.cpu().numpy(), ro.rewards.cpu().numpy()
    assert acts.shape == (nstep, n, 1) and acts.dtype == np.float32 and np.unique(acts).size > nstep
    twin = T.ControlTwin("Pendulum-v1", n, seed=seed)
    assert np.allclose(ro.obs_slots[0].cpu().numpy(), T.observe(T.PENDULUM, twin.state), rtol=0, atol=F32_ULP2)
    for t in range(nstep):
        exp = twin.step(acts[t])
        # a free run of 8 steps: the f64 reward drifts far less than an f32 ulp, so the f32 casts stay within one
        assert _ulps_f32(rews[t], exp["reward"]).max() <= 1, t
    assert np.abs(env.state.cpu().numpy() - twin.state).max() <= 1e-12
    # and the action matters: other torques from the same state give other rewards
    other = T.ControlTwin("Pendulum-v1", n, seed=seed).step(np.zeros((n, 1), np.float32))["reward"]
    assert (other != rews[0]).any()


def test_vecnormalize_wraps_the_control_env():
    """make_env(dynamics="real") wraps the control env in VecNormalize as the synthetic one: the physics state
    lives in the env, so the wrapper's in-place step over its raw buffer leaves the dynamics untouched."""
    import env as E
    n, seed = 16, 8
    wrapped = E.make_env("Acrobot-v1", n_envs=n, seed=seed, dynamics="real")
    bare = E.make_env("Acrobot-v1", n_envs=n, seed=seed, dynamics="real", normalize=False)
    assert isinstance(wrapped, E.VecNormalize) and isinstance(wrapped.venv, E.DeviceControlEnv)
    assert isinstance(bare, E.DeviceControlEnv)
    assert type(E.make_env("Acrobot-v1", n_envs=n, seed=seed).venv) is E.DeviceVecEnv  # the default is unchanged
    wrapped.reset()
    bare.reset()
    for t in range(1, 21):
        a = _dev(T.draw_actions("Acrobot-v1", seed, np.arange(n), t))
        o, _, d, _ = wrapped.step(a)
        ob, _, db, _ = bare.step(a)
        assert torch.equal(wrapped.raw, ob) and torch.equal(d, db) and torch.equal(wrapped.venv.state, bare.state)
        assert float(o.abs().max()) <= 10.0


def test_cartpole_learns():
    """PPO raises CartPole's episode return: the mean of the last 50 episodes is at least 3x the mean of the
    first 50 (the untrained policy: ~22, as the twin's random policy; 3x is more than 20 standard errors above
    chance), and learn(reward_target=first mean x 3) stops early on merit.
    Measured on an MI355X: see DESIGN.md "Real-dynamics envs"."""
    import ppo
    _quiet("PPO", "CartPole-v1")
    np.random.seed(0)
    torch.manual_seed(0)
    kw = dict(env_id="CartPole-v1", dynamics="real", n_envs=64, nstep=128, batch_size=1024, n_epochs=4, lr=1e-3,
              hidden_size=64, seed=0, quiet=True)
    alg = ppo.PPO(**kw)
    t0 = time.time()
    first, seen, last = [], 0, None
    for it in range(LEARN_ITERS):
        alg.collect_samples()
        ret = alg.rollout.done_ret.cpu().numpy()
        fin = ret[~np.isnan(ret)]  # row-major over (t, env): the order episodes finished in
        if len(first) < 50:
            first.extend(fin[:50 - len(first)].tolist())
        seen += fin.size
        alg.train()
    last = float(np.mean([e["r"] for e in alg.ep_info_buffer]))
    first_mean = float(np.mean(first))
    torch.cuda.synchronize()
    print(f"CartPole-v1 PPO: first-50 mean return {first_mean:.1f}, last-50 mean {last:.1f} after {LEARN_ITERS} "
          f"iterations ({alg.num_timesteps} steps, {seen} episodes), {time.time() - t0:.1f} s")
    assert len(first) == 50 and len(alg.ep_info_buffer) == 50
    assert 15.0 <= first_mean <= 30.0  # an untrained policy plays like a random one
    assert last >= 3.0 * first_mean

    np.random.seed(0)
    torch.manual_seed(0)
    alg = ppo.PPO(**kw)
    total = LEARN_ITERS * 128 * 64
    alg.learn(total_timesteps=total, log_interval=None, reward_target=3.0 * first_mean)
    print(f"learn(reward_target={3.0 * first_mean:.1f}) returned after {alg.num_timesteps} of {total} steps")
    assert alg.num_timesteps < total
    assert np.mean([e["r"] for e in alg.ep_info_buffer]) > 3.0 * first_mean

