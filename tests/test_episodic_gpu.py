"""The episodic novelty bonus on the device (csrc/episodic.hip, ppox_simhash_sums_u8, RolloutStorage.episodic,
PPO(episodic=True)) against the numpy twin (tests/episodic_twin.py).  The embeddings and squared distances are
integers and every float64 operation is done in a stated order, so every comparison is bit for bit."""
import functools
import os

import numpy as np
import pytest
import torch

import episodic_twin as T
import simhash_px_twin as H

pytestmark = pytest.mark.gpu

FRAME = 84 * 84
STACK = 4 * FRAME


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


@functools.lru_cache(maxsize=None)
def twin_matrix(D, seed):
    A = H.matrix(D, seed)
    A.setflags(write=False)
    return A


def _device_matrix(D, seed):
    import native
    A8 = torch.empty((16, D), dtype=torch.int8, device="cuda")
    rowsum = torch.empty(16, dtype=torch.int32, device="cuda")
    native.simhash_matrix_i8(D, seed, A8, rowsum)
    return A8, rowsum


def _device_sums_and_keys(x, D, A8, rowsum):
    """(sums (N, 16), keys (N,)) of the rows of the device uint8 view x (rows at x.stride(0))."""
    import native
    N = x.shape[0]
    ws = torch.empty(native.simhash_keys_u8_workspace_bytes(N) // 4, dtype=torch.int32, device="cuda")
    sums = torch.full((N, 16), -7, dtype=torch.int32, device="cuda")
    keys = torch.full((N,), -1, dtype=torch.int32, device="cuda")
    native.simhash_sums_u8(x, N, D, x.stride(0), A8, rowsum, ws, sums)
    native.simhash_keys_u8(x, N, D, x.stride(0), A8, rowsum, ws, keys)
    return sums.cpu().numpy(), keys.cpu().numpy()


# ------------------------------------------------------------------------------------------------------ sums
@pytest.mark.parametrize("D", [16, 17, FRAME, STACK])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 130])
def test_sums_equal_twin_and_their_signs_are_the_keys(N, D):
    seed = 7
    A = twin_matrix(D, seed)
    A8, rowsum = _device_matrix(D, seed)
    rs = np.random.RandomState(N * 1000 + D % 997)
    x = rs.randint(0, 256, (N, D)).astype(np.uint8)
    x[0] = 0                                    # frames of all 0 and all 255 (one row each; N = 1: the 255s)
    x[N - 1] = 255
    sparse = (rs.rand(N, D) < 0.01).astype(np.uint8) * 255      # mostly-black frames, as the envs draw them
    for name, data in (("random", x), ("zeros", np.zeros((N, D), np.uint8)), ("ones255", np.full((N, D), 255, np.uint8)),
                       ("sparse", sparse)):
        exp = T.sums(data, A)
        got, keys = _device_sums_and_keys(torch.from_numpy(data).cuda(), D, A8, rowsum)
        assert _same(got, exp), name
        packed = ((got > 0).astype(np.int64) << np.arange(16)).sum(axis=1).astype(np.int32)
        assert np.array_equal(packed, keys) and np.array_equal(keys, H.keys(data, A)), name
    assert (T.sums(np.zeros((1, D), np.uint8), A) == 0).all()
    assert np.array_equal(T.sums(np.full((1, D), 255, np.uint8), A)[0], 255 * A.astype(np.int64).sum(axis=1))


@pytest.mark.parametrize("N", [1, 65])
def test_sums_of_the_newest_frame_read_in_place(N):
    """obs_stride > D and the pointer at frame 3 of each stack: the MFMA kernel on a strided view (21,168 and
    28,224 are multiples of 16), and the plain kernel on a view one byte further."""
    A = twin_matrix(FRAME, 3)
    A8, rowsum = _device_matrix(FRAME, 3)
    rs = np.random.RandomState(N)
    stacks = rs.randint(0, 256, (N, STACK + 16)).astype(np.uint8)
    dev = torch.from_numpy(stacks).cuda()
    for off in (3 * FRAME, 3 * FRAME + 1):
        view = dev[:, off:off + FRAME]
        assert view.stride(0) == STACK + 16 and (view.data_ptr() % 16 == 0) == (off % 16 == 0)
        got, keys = _device_sums_and_keys(view, FRAME, A8, rowsum)
        assert _same(got, T.sums(stacks[:, off:off + FRAME], A)), off
        assert np.array_equal(keys, H.keys(stacks[:, off:off + FRAME], A))


def test_argument_checks_come_before_any_launch():
    import native
    lib = native.load()
    assert lib.ppox_simhash_sums_u8(None, 0, 0, 0, None, None, None, None, None) == 0      # N == 0: OK, as the keys
    assert lib.ppox_simhash_sums_u8(None, 4, 16, 16, None, None, None, None, None) == -1000
    assert b"null pointer" in lib.ppox_last_error()
    x = torch.zeros(64, dtype=torch.int32, device="cuda")
    p = x.data_ptr()
    assert lib.ppox_simhash_sums_u8(p, 4, 16, 8, p, p, p, p, None) == -1000                # stride < D
    assert lib.ppox_episodic_knn(None, None, 4, 4, 4, None, None, None, None, None, None) == -1000
    assert b"null pointer" in lib.ppox_last_error()
    for N, L, K in ((0, 4, 4), (4, 0, 4), (4, 4, 0), (4, 4, 17), (2 ** 31, 4, 4)):
        assert lib.ppox_episodic_knn(p, p, N, L, K, p, p, p, p, p, None) == -1000, (N, L, K)
    assert lib.ppox_episodic_reward(None, None, None, 4, 4, None, .99, .1, 1e-3, 8e-3, 1e-3, 8., None, None,
                                    None) == -1000
    for N, K in ((0, 4), (4, 0), (4, 17)):
        assert lib.ppox_episodic_reward(p, p, p, N, K, p, .99, .1, 1e-3, 8e-3, 1e-3, 8., p, p, None) == -1000


# ------------------------------------------------------------------------------------------- memory and bonus
@pytest.mark.parametrize("case", T.CASES, ids=T.case_id)
def test_memory_and_bonus_equal_twin_at_every_step(case):
    """3 L + 2 steps of knn -> reward on the device against the twin: mem, count, dm, dk (masked by kfound),
    kfound, mk, bonus and rewards after every step, and the branches the case is there for were reached."""
    import native
    N, L, K = case["N"], case["L"], case["K"]
    emb, done, rew = T.case_inputs(case)
    tw = T.Episodic(N, L, K, smax=case["smax"])
    d = "cuda"
    mem = torch.zeros((N, L, 16), dtype=torch.int32, device=d)
    count = torch.zeros(N, dtype=torch.int32, device=d)
    dm = torch.zeros(2, dtype=torch.float64, device=d)
    dk = torch.full((N, K), -1.0, dtype=torch.float64, device=d)
    kfound = torch.full((N,), -1, dtype=torch.int32, device=d)
    mk = torch.full((N,), -1.0, dtype=torch.float64, device=d)
    bonus = torch.full((N,), -1.0, device=d)
    emb_d, done_d, rew_d = (torch.from_numpy(a).cuda() for a in (emb, done, rew))
    for t in range(len(emb)):
        e_dk, e_kf, e_mk = tw.knn_step(emb[t], done[t])
        e_rew, e_bonus = tw.reward_step(e_dk, e_kf, e_mk, rew[t])
        native.episodic_knn(emb_d[t], done_d[t], N, L, K, mem, count, dk, kfound, mk)
        native.episodic_reward(dk, kfound, mk, N, K, dm, tw.decay, tw.beta, tw.eps, tw.xi, tw.c, tw.smax, rew_d[t],
                               bonus)
        g_kf = kfound.cpu().numpy()
        assert _same(g_kf, e_kf), t
        live = np.arange(K)[None, :] < e_kf[:, None]
        assert _same(np.where(live, dk.cpu().numpy(), 0.0), e_dk), t
        assert _same(mk.cpu().numpy(), e_mk), t
        assert _same(mem.cpu().numpy(), tw.mem) and _same(count.cpu().numpy(), tw.count), t
        assert _same(dm.cpu().numpy(), tw.dm), t
        assert _same(bonus.cpu().numpy(), e_bonus) and _same(rew_d[t].cpu().numpy(), e_rew), t
    missing = [b for b in T.case_branches(case) if tw.seen[b] == 0]
    assert not missing, (missing, tw.seen)
    if case["kind"] == "identical":
        assert tw.dm[0] == 0 and tw.dm[1] > 0 and float(dm[0]) == 0


# -------------------------------------------------------------------------------------------------- algorithm
CFG = dict(n_envs=8, nstep=16, batch_size=64, n_epochs=1, quiet=True, dynamics="real")
ENVS = {"KeyDoor-v0": dict(seed=11, max_len=5), "Catch-v0": dict(seed=3, max_len=None)}


def _quiet(env_id):
    import logger
    logger.configure("PPO", env_id, quiet=True)


def _make(env_id, graph=None, **kw):
    import env as E
    import ppo
    spec = ENVS[env_id]
    if graph is not None:
        os.environ["PPOX_COLLECT_GRAPH"] = "1" if graph else "0"
    try:
        np.random.seed(0)
        torch.manual_seed(0)
        if spec["max_len"] is not None:
            kw["env"] = E.make_env(env_id, n_envs=8, seed=spec["seed"], dynamics="real", max_len=spec["max_len"])
        return ppo.PPO(env_id=env_id, seed=spec["seed"], **CFG, **kw)
    finally:
        os.environ.pop("PPOX_COLLECT_GRAPH", None)


def _collect3(alg):
    outs = []
    for _ in range(3):
        alg.collect_samples()
        ro = alg.rollout
        rec = dict(actions=ro.actions, rewards=ro.rewards, values=ro.values, log_probs=ro.log_probs, masks=ro.masks,
                   obs_slots=ro.obs_slots, advantages=ro.advantages)
        if ro.do_episodic:
            rec.update(bonus=ro.episodic_bonus, mem=ro.mem, count=ro.count, dm=ro.dm)
        outs.append({k: v.cpu().numpy().copy() for k, v in rec.items()})
    return outs


@functools.lru_cache(maxsize=None)
def _plain_rollouts(env_id):
    """Three consecutive collects of a default-constructed PPO (no train() in between: the policy stands still, so
    a PPO with the bonus on the same seeds sees the same frames, masks and env rewards)."""
    return _collect3(_make(env_id, graph=False))


@pytest.mark.parametrize("frames", ["last", "stack"])
@pytest.mark.parametrize("env_id", list(ENVS))
def test_ppo_episodic_equals_twin_replay_eager_and_graphed(env_id, frames):
    """8 envs x 16 steps, three collects: every env finishes episodes inside a rollout (KeyDoor at max_len 5,
    Catch every 11 steps) and the state crosses two rollout boundaries.  Rewards and episodic_bonus == the twin's
    replay of the recorded frames and masks, the captured-graph collect == the eager one, bit for bit."""
    _quiet(env_id)
    plain = _plain_rollouts(env_id)
    kw = dict(episodic=True, episodic_kwargs=dict(frames=frames, k=3))
    ea, ga = _make(env_id, graph=False, **kw), _make(env_id, graph=True, **kw)
    eager, graphed = _collect3(ea), _collect3(ga)
    assert ga._collect_graph_ok() and not ea._collect_graph_ok() and ea._cgraph is None and ga._cgraph is not None
    ro = ea.rollout
    L = ENVS[env_id]["max_len"] or 256
    assert (ro.epi_capacity, ro.epi_k, ro.epi_frames, ro.epi_D) == (L, 3, frames, FRAME if frames == "last" else STACK)
    assert ro.epi_seed == ENVS[env_id]["seed"] and ro.episodic_bonus.shape == (16, 8)
    A = twin_matrix(ro.epi_D, ro.epi_seed)
    tw = T.Episodic(8, L, K=3)
    for i in range(3):
        for k in ("actions", "values", "log_probs", "masks", "obs_slots"):   # the bonus changes the rewards only
            assert _same(eager[i][k], plain[i][k]), (i, k)
        assert eager[i]["masks"].sum() > 0 and eager[i]["masks"].any(axis=0).all()
        e_rew, e_bonus = T.replay(tw, A, frames, eager[i]["obs_slots"][:16], eager[i]["masks"], plain[i]["rewards"])
        assert _same(eager[i]["rewards"], e_rew) and _same(eager[i]["bonus"], e_bonus), i
        assert _same(eager[i]["mem"], tw.mem) and _same(eager[i]["count"], tw.count) and _same(eager[i]["dm"], tw.dm)
        assert not _same(eager[i]["rewards"], plain[i]["rewards"]) and (e_bonus > 0).any()
        for k in eager[i]:
            assert _same(eager[i][k], graphed[i][k]), (i, k)
    assert tw.seen["reset"] >= 8 and tw.dm[1] > 16
    if ENVS[env_id]["max_len"] is None:
        # Catch's episodes of 11 steps began before the rollout boundary and ended after it: the memory carried over
        assert (eager[0]["count"] > 0).all() and (eager[0]["count"] == 16 - 11).all()


def test_default_ppo_is_unchanged_and_learn_logs_the_two_keys(monkeypatch):
    import logger
    import ppo
    _quiet("KeyDoor-v0")
    for a, b in zip(_collect3(_make("KeyDoor-v0")), _plain_rollouts("KeyDoor-v0")):
        for k in b:
            assert _same(a[k], b[k]), k                  # two default-constructed PPOs, graph and eager: the same bits
    plain = _make("KeyDoor-v0")
    assert not plain.rollout.do_episodic and not plain.episodic and not hasattr(plain.rollout, "mem")
    dumps = []
    real_dump = logger.dump
    monkeypatch.setattr(logger, "dump", lambda step=0: (dumps.append(logger.get_values()), real_dump(step)))
    alg = _make("KeyDoor-v0", episodic=True)
    assert alg.rollout.epi_capacity == 5 and alg.rollout.epi_k == 10 and alg.rollout.epi_frames == "last"
    alg.learn(total_timesteps=8 * 16, log_interval=1)
    torch.cuda.synchronize()
    assert len(dumps) == 1 and alg._n_updates == 1
    bonus, dm = dumps[0]["rollout/episodic_bonus"], dumps[0]["rollout/episodic_dm"]
    assert np.isfinite(bonus) and np.isfinite(dm) and bonus > 0 and dm > 0
    assert bonus == float(alg.rollout.episodic_bonus.mean().item()) and dm == float(alg.rollout.dm[0].item())
    assert np.isfinite(alg.flat.data.detach().cpu().numpy()).all()
    plain.learn(total_timesteps=8 * 16, log_interval=1)
    assert len(dumps) == 2 and not [k for k in dumps[1] if "episodic" in k]


def test_refused_combinations_and_keywords():
    import buffer
    import env as E
    import ppo
    kd = dict(env_id="KeyDoor-v0", **CFG)
    with pytest.raises(NotImplementedError, match="sil"):
        ppo.PPO(episodic=True, sil=True, **kd)
    with pytest.raises(NotImplementedError, match="sim_hash"):
        ppo.PPO(episodic=True, sim_hash=True, **kd)
    with pytest.raises(NotImplementedError, match="PPO_RND"):
        ppo.PPO_RND(episodic=True, **kd)
    with pytest.raises(NotImplementedError, match="PPO_ICM"):
        ppo.PPO_ICM(episodic=True, **kd)
    with pytest.raises(NotImplementedError, match="uint8"):
        ppo.PPO(env_id="CartPole-v1", episodic=True, **CFG)
    with pytest.raises(TypeError, match="capacity.*frames"):
        ppo.PPO(episodic=True, episodic_kwargs=dict(kk=3), **kd)
    with pytest.raises(ValueError, match="frames"):
        ppo.PPO(episodic=True, episodic_kwargs=dict(frames="first"), **kd)
    with pytest.raises(ValueError, match="k must lie"):
        ppo.PPO(episodic=True, episodic_kwargs=dict(k=17), **kd)
    box = E.Box((4, 84, 84), 0, 255, np.uint8)
    with pytest.raises(NotImplementedError, match="sim_hash"):
        buffer.RolloutStorage(4, 2, box, E.Discrete(3), sim_hash=True, episodic={})
    with pytest.raises(NotImplementedError, match="uint8"):
        buffer.RolloutStorage(4, 2, E.Box((4, 84, 84)), E.Discrete(3), episodic={})
    st = buffer.RolloutStorage(4, 2, box, E.Discrete(3), episodic=dict(capacity=7, beta=0.5))
    assert st.mem.shape == (2, 7, 16) and st.epi_coef == (0.99, 0.5, 1e-3, 8e-3, 1e-3, 8.0)
    st.count.fill_(3)
    st.reset()
    assert st.count.tolist() == [3, 3]                   # the episodic state outlives reset()


def test_episodic_refused_under_a_process_group(monkeypatch):
    import ppo
    from dist import DistContext

    class Ctx:
        enabled, rank, world = True, 0, 2
    monkeypatch.setattr(DistContext, "current", staticmethod(lambda: Ctx()))
    with pytest.raises(NotImplementedError, match="process group"):
        ppo.PPO(env_id="KeyDoor-v0", episodic=True, **CFG)
