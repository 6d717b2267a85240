"""KeyDoor-v0 on the device (csrc/env_grid.hip, env.DeviceKeyDoorEnv) against its numpy twin
(tests/keydoor_twin.py), through the public class and the algorithm constructors.  Everything
compared is integers and copied bytes: the tolerance is zero throughout."""
import os

import numpy as np
import pytest
import torch

import keydoor_twin as K

pytestmark = pytest.mark.gpu

N_ENVS, T_STEPS, MAX_LEN, SEED = K.PARITY_N, K.PARITY_T, K.PARITY_MAX_LEN, K.PARITY_SEED
SHARD_SEED = K.GPU_TEST_SEEDS[1]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _step_buffers(n):
    return dict(rewards=torch.empty(n, device="cuda"), dones=torch.empty(n, dtype=torch.uint8, device="cuda"),
                done_ret=torch.empty(n, device="cuda"), done_len=torch.empty(n, dtype=torch.int32, device="cuda"))


def _quiet(algo, env_id="KeyDoor-v0"):
    import logger
    logger.configure(algo, env_id, quiet=True)


def test_step_matches_twin_teacher_forced():
    """N = 67, T = 64, max_len = 40, the mixed action stream: at every step the twin starts from the device's
    downloaded state, episode index, bookkeeping and frame stack, and the next state, episode index, all four
    frames, rewards, dones, done_ret, done_len, ep_ret and ep_len are bit-exact; so is `visits` after the run.
    A few actions are set outside 0..4 on the way (they are stay).  test_keydoor_twin.py shows on the CPU that this
    run takes every branch at least three times; the counts are asserted here as well."""
    import env as E
    n = N_ENVS
    dev = E.make_env("KeyDoor-v0", n_envs=n, seed=SEED, dynamics="real", max_len=MAX_LEN)
    twin = K.KeyDoorTwin(n, seed=SEED, max_len=MAX_LEN)
    policy, _ = K.bfs_policy(twin.layout)
    assert type(dev) is E.DeviceKeyDoorEnv and dev.action_space.n == 5 and dev.max_len == MAX_LEN
    assert dev.observation_space.shape == (4, 84, 84) and dev.obs_dtype == torch.uint8
    assert dev.layout == twin.layout
    assert dev.visits.dtype == torch.int64 and tuple(dev.visits.shape) == (2, 12, 12)
    assert dev.state.dtype == torch.int32 and tuple(dev.state.shape) == (n, 4) and dev.episode.dtype == torch.int32
    obs = torch.full((n, 4, 84, 84), 77, dtype=torch.uint8, device="cuda")
    dev.reset_into(obs)
    assert np.array_equal(obs.cpu().numpy(), twin.obs)
    assert np.array_equal(dev.state.cpu().numpy(), twin.state)
    assert (dev.episode == 0).all() and (dev.ep_len == 0).all() and (dev.ep_ret == 0).all()
    assert np.array_equal(dev.visits.cpu().numpy(), twin.visits) and dev.coverage() == np.count_nonzero(twin.visits)
    nxt = torch.full_like(obs, 77)
    b = _step_buffers(n)
    for t in range(1, T_STEPS + 1):
        twin.state, twin.episode = dev.state.cpu().numpy(), dev.episode.cpu().numpy()
        twin.ep_ret, twin.ep_len = dev.ep_ret.cpu().numpy(), dev.ep_len.cpu().numpy()
        twin.obs = obs.cpu().numpy()
        a = K.draw_actions(SEED, twin.gids, t, twin.state, policy)
        if t % 16 == 5:
            a[1], a[3], a[5] = 5, -1, 2 ** 31 - 1
        dev.step_into(obs, nxt, _dev(a), b["rewards"], b["dones"], b["done_ret"], b["done_len"])
        exp = twin.step(a)
        done = b["dones"].cpu().numpy().astype(bool)
        assert np.array_equal(done, exp["done"]), t
        assert np.array_equal(dev.state.cpu().numpy(), twin.state), t
        assert np.array_equal(dev.episode.cpu().numpy(), twin.episode), t
        got = nxt.cpu().numpy()
        assert np.array_equal(got, exp["obs"]), t
        assert np.array_equal(b["rewards"].cpu().numpy(), exp["reward"]), t
        assert np.array_equal(b["done_ret"].cpu().numpy(), exp["done_ret"], equal_nan=True), t
        assert np.array_equal(b["done_len"].cpu().numpy(), exp["done_len"]), t
        assert np.array_equal(dev.ep_ret.cpu().numpy(), twin.ep_ret), t
        assert np.array_equal(dev.ep_len.cpu().numpy(), twin.ep_len), t
        if done.any():  # stack zeroed, the new episode's first frame last
            assert (got[done, :3] == 0).all() and (got[done, 3] == K.frame(twin.state[done], twin.layout)).all()
        obs, nxt = nxt, obs
    print("KeyDoor teacher-forced run events:", twin.counts)
    assert all(count >= 3 for count in twin.counts.values()), twin.counts
    assert np.array_equal(dev.visits.cpu().numpy(), twin.visits)
    resets = twin.counts["goals"] + twin.counts["time_limits"]
    assert int(dev.visits.sum()) == n * T_STEPS + n + resets
    assert dev.coverage() == np.count_nonzero(twin.visits) > 100


def test_step_in_place_matches_two_buffers():
    """obs_in == obs_out (the form VecEnv-style callers may use) writes the same stacks as two buffers."""
    import env as E
    n, steps = 5, 30
    envs = [E.DeviceKeyDoorEnv(n_envs=n, seed=SEED, env_offset=2, max_len=9) for _ in range(2)]
    a_obs = torch.empty((n, 4, 84, 84), dtype=torch.uint8, device="cuda")
    b_obs, b_nxt = torch.empty_like(a_obs), torch.empty_like(a_obs)
    envs[0].reset_into(a_obs)
    envs[1].reset_into(b_obs)
    ba, bb = _step_buffers(n), _step_buffers(n)
    for t in range(1, steps + 1):
        a = _dev(K.draw_actions(SEED, np.arange(2, 2 + n), t))
        envs[0].step_into(a_obs, a_obs, a, ba["rewards"], ba["dones"])
        envs[1].step_into(b_obs, b_nxt, a, bb["rewards"], bb["dones"])
        assert torch.equal(a_obs, b_nxt) and torch.equal(ba["dones"], bb["dones"]), t
        b_obs, b_nxt = b_nxt, b_obs
    assert torch.equal(envs[0].visits, envs[1].visits) and (envs[0].episode >= 3).all()


def _sharded_run(sizes, steps, seed, max_len):
    import env as E
    policy, _ = K.bfs_policy(K.layout(seed))
    outs, tables, off = [], [], 0
    for n in sizes:
        dev = E.DeviceKeyDoorEnv(n_envs=n, seed=seed, env_offset=off, max_len=max_len)
        gids = np.arange(off, off + n)
        obs = dev.reset()
        rows = [(obs.clone(), None, None)]
        for t in range(1, steps + 1):
            a = K.draw_actions(seed, gids, t, dev.state.cpu().numpy(), policy)
            obs, rew, done, _ = dev.step(_dev(a))
            rows.append((obs.clone(), rew.clone(), done.clone()))
        outs.append(rows)
        tables.append(dev.visits.clone())
        off += n
    return outs, tables


def test_sharding_never_changes_the_data():
    """Envs [0, 67) as one object == the same envs as three objects at env_offset 0 / 23 / 46, bit for bit, and
    the three visits tables sum to the one-shard table."""
    steps = 40
    (whole,), (table,) = _sharded_run([67], steps, SHARD_SEED, 25)
    parts, tables = _sharded_run([23, 23, 21], steps, SHARD_SEED, 25)
    n_done = 0
    for t in range(steps + 1):
        for k in range(3):
            if whole[t][k] is None:
                continue
            assert torch.equal(whole[t][k], torch.cat([p[t][k] for p in parts])), (t, k)
        n_done += 0 if whole[t][2] is None else int(whole[t][2].sum())
    assert n_done >= 67  # episodes ended and restarted on the way
    assert torch.equal(table, tables[0] + tables[1] + tables[2])
    assert int(table.sum()) == 67 * steps + 67 + n_done


def _same_bits(u, v):
    """torch.equal on the bit patterns (done_ret holds NaNs where no episode ended)."""
    if u.dtype == torch.float32:
        u, v = u.view(torch.int32), v.view(torch.int32)
    return torch.equal(u, v)


def test_keydoor_collect_graph_matches_eager():
    """The captured collect loop accepts the env (a DeviceAtariEnv): two collects replayed from the graph == two
    eager ones (PPOX_COLLECT_GRAPH=0) in a fresh object with the same seed, bit for bit, `visits` included.
    max_len = 12, so every env's episode ends inside each rollout of 16 steps."""
    import env as E
    import ppo
    _quiet("PPO")

    def run(graph):
        os.environ["PPOX_COLLECT_GRAPH"] = "1" if graph else "0"
        try:
            np.random.seed(0)
            torch.manual_seed(0)
            env = E.make_env("KeyDoor-v0", n_envs=8, seed=SEED, dynamics="real", max_len=12)
            alg = ppo.PPO(env_id="KeyDoor-v0", dynamics="real", n_envs=8, nstep=16, batch_size=64, n_epochs=1,
                          quiet=True, seed=SEED, env=env)
        finally:
            del os.environ["PPOX_COLLECT_GRAPH"]
        outs = []
        for _ in range(2):
            alg.collect_samples()
            ro = alg.rollout
            outs.append([x.clone() for x in (ro.actions, ro.rewards, ro.values, ro.log_probs, ro.masks, ro.obs_slots,
                                             ro.done_ret, ro.done_len, alg.env.state, alg.env.episode,
                                             alg.env.visits)])
        return alg, outs

    (ea, a), (ga, g) = run(False), run(True)
    assert type(ga.env).__name__ == "DeviceKeyDoorEnv" and ga._collect_graph_ok() and not ea._collect_graph_ok()
    assert ea._cgraph is None and ga._cgraph is not None
    for xa, xg in zip(a, g):
        for u, v in zip(xa, xg):
            assert _same_bits(u, v)
    masks = torch.cat([g[0][4], g[1][4]])  # 32 steps at max_len 12: every env ends at least twice
    assert int(masks.sum()) >= 16
    assert int(g[1][10].sum()) == 8 * 32 + 8 + int(masks.sum())  # visits: steps + first starts + restarts
    assert set(torch.cat([g[0][1], g[1][1]]).flatten().tolist()) <= {0.0, 1.0}


# name -> class, keywords, max_len (None: the constructor makes the env itself, max_len 200).  Self-imitation trains
# only once more than 100 ring rows belong to finished episodes: max_len = 8 ends every episode inside the rollout
ALGOS = {
    "PPO": ("PPO", {}, None),
    "PPO_SimHash": ("PPO", dict(sim_hash=True), None),
    "PPO_SIL": ("PPO", dict(sil=True, sil_kwargs=dict(size=1024, batch=32, epochs=1)), 8),
    "PPO_RND": ("PPO_RND", {}, None),
    "PPO_ICM": ("PPO_ICM", {}, None),
}


@pytest.mark.parametrize("name", list(ALGOS))
def test_algorithms_take_the_env_and_log_coverage(name, monkeypatch):
    """learn() for exactly one collect_samples() + train() (8 envs x 16 steps, batch 32, one epoch) of every
    algorithm on KeyDoor-v0: the env is the device gridworld, the losses are finite, the ICM run takes the native
    path, and the log point holds rollout/coverage == count_nonzero(env.visits)."""
    import logger
    import ppo
    import env as E
    cls, kw, max_len = ALGOS[name]
    if max_len is not None:
        kw = dict(kw, env=E.make_env("KeyDoor-v0", n_envs=8, seed=SEED, dynamics="real", max_len=max_len))
    dumps = []
    real_dump = logger.dump

    def dump(step=0):
        dumps.append(logger.get_values())
        real_dump(step)

    monkeypatch.setattr(logger, "dump", dump)
    np.random.seed(0)
    torch.manual_seed(0)
    alg = getattr(ppo, cls)(env_id="KeyDoor-v0", dynamics="real", n_envs=8, nstep=16, batch_size=32, n_epochs=1,
                            quiet=True, seed=SEED, **kw)
    assert type(alg.env).__name__ == "DeviceKeyDoorEnv" and alg.env.max_len == (max_len or 200) and alg.n_actions == 5
    if cls == "PPO_ICM":
        assert alg._icm_native is not None
    alg.learn(total_timesteps=8 * 16, log_interval=1)
    torch.cuda.synchronize()
    assert alg.num_timesteps == 8 * 16 and alg._n_updates == 1 and len(dumps) == 1
    visits = alg.env.visits.cpu().numpy()
    assert visits.sum() == 8 * 16 + 8 + int(alg.rollout.masks.sum())
    assert dumps[0]["rollout/coverage"] == np.count_nonzero(visits) == alg.env.coverage() > 8
    logged = logger.get_values()  # train() runs after the log point: its records are still in the logger
    losses = {k: v for k, v in logged.items() if k.startswith("train/") and k.endswith("loss")}
    assert len(losses) >= 4 and all(np.isfinite(v) for v in losses.values()), losses
    assert np.isfinite(alg.flat.data.detach().cpu().numpy()).all()
    if name == "PPO_SimHash":
        assert alg.rollout.hash_px and float(alg.rollout.rewards.abs().sum()) > 0  # the count bonus reached the rewards
    if name == "PPO_SIL":
        assert "train/sil_loss" in logged and np.isfinite(logged["train/sil_loss"])
    if cls == "PPO_ICM":
        assert "train/icm_loss" in logged


def test_other_envs_log_no_coverage(monkeypatch):
    """No other env's log schema changes: a Catch run has no rollout/coverage key."""
    import logger
    import ppo
    dumps = []
    real_dump = logger.dump
    monkeypatch.setattr(logger, "dump", lambda step=0: (dumps.append(logger.get_values()), real_dump(step)))
    alg = ppo.PPO(env_id="Catch-v0", dynamics="real", n_envs=8, nstep=16, batch_size=32, n_epochs=1, quiet=True, seed=3)
    alg.learn(total_timesteps=8 * 16, log_interval=1)
    assert len(dumps) == 1 and "rollout/coverage" not in dumps[0] and "time/total timesteps" in dumps[0]
