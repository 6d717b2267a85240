"""The elliptical episodic bonus on the device (ppox_elliptical_bonus and ppox_ngu_modulate of csrc/episodic.hip,
RolloutStorage / IntrinsicStorage with kind="elliptical", PPO and PPO_NGU) against the numpy twins
(tests/elliptical_twin.py, tests/ngu_twin.py).  Every float64 operation is done in a stated order, so every
comparison is bit for bit."""
import functools
import os

import numpy as np
import pytest
import torch

import elliptical_twin as T
import episodic_twin as E
import ngu_twin as G
import simhash_px_twin as H

pytestmark = pytest.mark.gpu

FRAME = 84 * 84
STACK = 4 * FRAME
GUARD = -7.0
ELL = dict(kind="elliptical")


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


# ----------------------------------------------------------------------------------------------------- kernels
class _Dev:
    """ppox_elliptical_bonus's state and outputs with a guard row on either side of each."""

    def __init__(self, N, ridge, outputs):
        d = "cuda"
        self.N = N
        self.minv = torch.full((N + 2, 16, 16), GUARD, dtype=torch.float64, device=d)
        self.minv[1:N + 1] = torch.eye(16, dtype=torch.float64, device=d) * (1.0 / ridge)
        self.count = torch.full((N + 2,), -7, dtype=torch.int32, device=d)
        self.count[1:N + 1] = 0
        self.eb = torch.full((N + 2,), GUARD, dtype=torch.float64, device=d)
        self.out = torch.full((5, N), GUARD, device=d) if outputs else None   # guard, rewards, guard, bonus, guard

    def step(self, native, emb, done, ridge, beta, rewards=None):
        N = self.N
        if self.out is not None:
            self.out[1].copy_(rewards)
        native.elliptical_bonus(emb, done, N, ridge, beta, self.minv[1:N + 1], self.count[1:N + 1], self.eb[1:N + 1],
                                None if self.out is None else self.out[1], None if self.out is None else self.out[3])

    def check(self, tw, t):
        N = self.N
        minv, count, eb = self.minv.cpu().numpy(), self.count.cpu().numpy(), self.eb.cpu().numpy()
        assert _same(minv[1:N + 1], tw.minv), t
        assert _same(count[1:N + 1], tw.count) and _same(eb[1:N + 1], tw.eb), t
        assert (minv[[0, N + 1]] == GUARD).all() and (count[[0, N + 1]] == -7).all() and (eb[[0, N + 1]] == GUARD).all()


@pytest.mark.parametrize("case", T.gpu_cases(), ids=T.case_id)
def test_kernel_equals_twin_at_every_step(case):
    """12 steps of ppox_elliptical_bonus against the twin: minv, count, eb, bonus and rewards after every step,
    guard rows untouched; the same again with rewards = NULL, bonus = NULL (minv, count, eb)."""
    import native
    N, ridge, beta = case["N"], case["ridge"], 0.1
    emb, done, rew = (a[:T.GPU_STEPS] for a in E.case_inputs(case))
    tw = T.Elliptical(N, ridge, beta)
    full, bare = _Dev(N, ridge, True), _Dev(N, ridge, False)
    emb_d, done_d, rew_d = (torch.from_numpy(a).cuda() for a in (emb, done, rew))
    for t in range(len(emb)):
        e_rew, e_bonus = tw.step(emb[t], done[t], rew[t])
        full.step(native, emb_d[t], done_d[t], ridge, beta, rew_d[t])
        bare.step(native, emb_d[t], done_d[t], ridge, beta)
        full.check(tw, t)
        bare.check(tw, t)
        o = full.out.cpu().numpy()
        assert _same(o[1], e_rew) and _same(o[3], e_bonus), t
        assert (o[0::2] == GUARD).all(), t
        assert np.array_equal(tw.minv, tw.minv.transpose(0, 2, 1)) and np.isfinite(tw.minv).all(), t
    missing = [b for b in T.case_branches(case, done) if tw.seen[b] == 0]
    assert not missing, (missing, tw.seen)


MOD_CASES = [(kind, N) for kind in G.KINDS for N in (1, 65, 1025, 2500)]


@pytest.mark.parametrize("kind,N", MOD_CASES, ids=[f"{k}-N{n}" for k, n in MOD_CASES])
def test_ngu_modulate_equals_twin_and_ngu_reward(kind, N):
    """8 steps of ppox_ngu_modulate on a random float64 bonus: em, modulator, int_rewards and bonus == the twin;
    em and modulator == what ppox_ngu_reward makes of the same err stream from the same em (its kNN inputs
    empty: kfound = 0)."""
    import native
    case = dict(N=N, L=2, K=3, seed=500 + N, err=kind)
    err, warm, em0 = G.case_errors(case)
    S = len(err)
    rs = np.random.RandomState(N)
    eb = rs.rand(S, N) * np.exp(4 * rs.randn(S, N))
    eb[rs.rand(S, N) < 0.2] = 0.0
    tw = G.Ngu(N, 1, mod_max=G.MOD_MAX, em=em0)
    d = "cuda"
    em = torch.tensor(list(em0), dtype=torch.float64, device=d)
    em_ref = em.clone()
    out = torch.full((7, N), GUARD, device=d)                # guard, int_rewards, guard, bonus, guard, modulator, guard
    ref = torch.full((3, N), GUARD, device=d)
    kf = torch.zeros(N, dtype=torch.int32, device=d)
    z = torch.zeros((N, 3), dtype=torch.float64, device=d)
    mk, dm = torch.zeros(N, dtype=torch.float64, device=d), torch.zeros(2, dtype=torch.float64, device=d)
    eb_d, err_d = torch.from_numpy(eb).cuda(), torch.from_numpy(err).cuda()
    for t in range(S):
        e = None if t < warm else err[t]
        e_int, e_bonus, e_mod = T.modulate(tw, eb[t], e)
        e_d = None if t < warm else err_d[t]
        native.ngu_modulate(eb_d[t], e_d, N, em, G.MOD_MAX, out[1], out[3], out[5])
        native.ngu_reward(z, kf, mk, e_d, N, 3, dm, em_ref, .99, 1e-3, 8e-3, 1e-3, 8., G.MOD_MAX, ref[0], ref[1],
                          ref[2])
        o = out.cpu().numpy()
        assert _same(em.cpu().numpy(), tw.em), (t, em.cpu().numpy(), tw.em)
        assert _same(o[5], e_mod) and _same(o[1], e_int) and _same(o[3], e_bonus), t
        assert (o[0::2] == GUARD).all(), t
        assert _same(em_ref.cpu().numpy(), tw.em) and _same(ref[2].cpu().numpy(), e_mod), t
    assert tw.seen["warm"] == warm
    if kind == "const":
        assert tw.seen["sigma0"] == S * N
    else:
        assert tw.seen["lo"] + tw.seen["mid"] + tw.seen["hi"] == (S - warm) * N
        assert N == 1 or (tw.seen["lo"] >= 1 and tw.seen["mid"] >= 1)


def test_null_outputs_are_accepted_and_null_state_is_not():
    import native
    lib = native.load()
    x = torch.zeros(64, dtype=torch.float64, device="cuda")
    p = x.data_ptr()
    assert lib.ppox_elliptical_bonus(None, p, 1, 1.0, 0.1, p, p, p, p, p, None) == -1000
    assert lib.ppox_ngu_modulate(p, p, 1, None, 5.0, p, p, p, None) == -1000
    torch.cuda.synchronize()
    assert (x == 0).all()


# -------------------------------------------------------------------------------------------------- algorithms
CFG = dict(n_envs=8, nstep=16, batch_size=64, n_epochs=1, quiet=True, dynamics="real")
ENVS = {"KeyDoor-v0": dict(seed=11, max_len=5), "Catch-v0": dict(seed=3, max_len=None)}


def _make(cls_name, env_id, graph=None, **kw):
    import env as Env
    import logger
    import ppo
    logger.configure(cls_name, env_id, quiet=True)
    spec = ENVS[env_id]
    if graph is not None:
        os.environ["PPOX_COLLECT_GRAPH"] = "1" if graph else "0"
    try:
        np.random.seed(0)
        torch.manual_seed(0)
        if spec["max_len"] is not None:
            kw["env"] = Env.make_env(env_id, n_envs=8, seed=spec["seed"], dynamics="real", max_len=spec["max_len"])
        return getattr(ppo, cls_name)(env_id=env_id, seed=spec["seed"], **CFG, **kw)
    finally:
        os.environ.pop("PPOX_COLLECT_GRAPH", None)


_PLAIN = ("actions", "rewards", "values", "log_probs", "masks", "obs_slots", "advantages")


def _collect3(alg):
    outs = []
    for _ in range(3):
        alg.collect_samples()
        ro = alg.rollout
        rec = {k: getattr(ro, k) for k in _PLAIN}
        if ro.do_episodic and ro.epi_kind == "elliptical":
            rec.update(bonus=ro.episodic_bonus, minv=ro.minv, count=ro.count, emb=ro.epi_emb)
        elif ro.do_episodic:
            rec.update(bonus=ro.episodic_bonus, mem=ro.mem, count=ro.count, dm=ro.dm)
        outs.append({k: v.cpu().numpy().copy() for k, v in rec.items()})
    return outs


@functools.lru_cache(maxsize=None)
def _plain_rollouts(env_id):
    """Three consecutive collects of a default-constructed PPO (no train() in between: the policy stands still, so
    a PPO with the bonus on the same seeds sees the same frames, masks and env rewards)."""
    return _collect3(_make("PPO", env_id, graph=False))


@pytest.mark.parametrize("frames", ["last", "stack"])
@pytest.mark.parametrize("env_id", list(ENVS))
def test_ppo_elliptical_equals_twin_replay_eager_and_graphed(env_id, frames):
    """8 envs x 16 steps, three collects: episodes end inside the rollouts and the state crosses two rollout
    boundaries.  rewards, episodic_bonus, minv and count == the twin's replay of the recorded frames and masks, the
    captured-graph collect == the eager one, and the embeddings' signs are still the pixel hash's keys."""
    plain = _plain_rollouts(env_id)
    kw = dict(episodic=True, episodic_kwargs=dict(ELL, frames=frames))
    ea, ga = _make("PPO", env_id, graph=False, **kw), _make("PPO", env_id, graph=True, **kw)
    eager, graphed = _collect3(ea), _collect3(ga)
    assert ga._collect_graph_ok() and not ea._collect_graph_ok() and ea._cgraph is None and ga._cgraph is not None
    ro = ea.rollout
    D = FRAME if frames == "last" else STACK
    assert (ro.epi_kind, ro.epi_ridge, ro.epi_beta, ro.epi_frames, ro.epi_D) == ("elliptical", 2.0 ** 30, 0.1, frames, D)
    assert ro.epi_seed == ENVS[env_id]["seed"] and ro.episodic_bonus.shape == (16, 8)
    assert ro.minv.shape == (8, 16, 16) and ro.minv.dtype == torch.float64 and ro.eb.dtype == torch.float64
    for name in ("mem", "dm", "epi_dk", "epi_kfound", "epi_mk", "epi_capacity", "epi_k"):
        assert not hasattr(ro, name), name
    A = twin_matrix(D, ro.epi_seed)
    tw = T.Elliptical(8, 2.0 ** 30, 0.1)
    for i in range(3):
        for k in ("actions", "values", "log_probs", "masks", "obs_slots"):   # the bonus changes the rewards only
            assert _same(eager[i][k], plain[i][k]), (i, k)
        assert eager[i]["masks"].sum() > 0
        obs = eager[i]["obs_slots"]
        e_rew, e_bonus = T.replay(tw, A, frames, obs[:16], eager[i]["masks"], plain[i]["rewards"])
        assert _same(eager[i]["rewards"], e_rew) and _same(eager[i]["bonus"], e_bonus), i
        assert _same(eager[i]["minv"], tw.minv) and _same(eager[i]["count"], tw.count), i
        assert not _same(eager[i]["rewards"], plain[i]["rewards"]) and (e_bonus > 0).any()
        last = obs[15][:, -1] if frames == "last" else obs[15]
        packed = ((eager[i]["emb"] > 0).astype(np.int64) << np.arange(16)).sum(axis=1).astype(np.int32)
        assert np.array_equal(packed, H.keys(last.reshape(8, -1), A)), i
        for k in eager[i]:
            assert _same(eager[i][k], graphed[i][k]), (i, k)
    assert tw.seen["reset"] >= 8 and tw.seen["first_step"] >= 16 and tw.seen["fresh"] + tw.seen["in_span"] > 0
    ro.count.fill_(3)
    ro.reset()
    assert ro.count.tolist() == [3] * 8                      # the state outlives reset()


_SHARED = ("rewards", "masks", "actions", "values", "obs_slots")


@pytest.mark.parametrize("frames", ["last", "stack"])
@pytest.mark.parametrize("env_id", list(ENVS))
def test_ppo_ngu_elliptical_equals_twin_replay_over_three_collects(env_id, frames):
    """PPO_NGU with kind="elliptical", rnd_start = 4: em after every step, int_rewards, episodic_bonus,
    ngu_modulator, minv and count == the replay; the env's stream == a PPO_RND's on the same seeds."""
    ngu = _make("PPO_NGU", env_id, rnd_start=4, episodic_kwargs=dict(ELL, frames=frames))
    rnd = _make("PPO_RND", env_id, rnd_start=4)
    ro = ngu.rollout
    D = FRAME if frames == "last" else STACK
    assert (ro.epi_kind, ro.epi_ridge, ro.epi_frames, ro.epi_D, ro.ngu_mod_max) == ("elliptical", 2.0 ** 30, frames, D, 5.)
    assert ro.em.tolist() == list(G.EM_START) and not hasattr(ro, "mem") and not hasattr(ro, "dm")
    ems, real_ngu = [], ro.ngu

    def recording_ngu(obs, dones, err, t=None):
        out = real_ngu(obs, dones, err, t)
        ems.append((err is None, ro.em.clone()))
        return out
    ro.ngu = recording_ngu
    A = twin_matrix(D, ro.epi_seed)
    tw = T.NguElliptical(8, 2.0 ** 30)
    any_mod = False
    for i in range(3):
        ngu.collect_samples()
        rnd.collect_samples()
        for k in _SHARED:                                   # the bonus leaves the env's stream as it is
            assert _same(getattr(ro, k).cpu().numpy(), getattr(rnd.rollout, k).cpu().numpy()), (i, k)
        warm = np.array([w for w, _ in ems[16 * i:]])
        assert warm.tolist() == ([True] * 3 + [False] * 13 if i == 0 else [False] * 16)
        obs, masks, err = ro.obs_slots.cpu().numpy(), ro.masks.cpu().numpy(), ro.rnd_err.cpu().numpy()
        assert masks.sum() > 0
        e_int = np.empty((16, 8), np.float32)
        e_bonus, e_mod = np.empty_like(e_int), np.empty_like(e_int)
        for t in range(16):                                 # one step at a time, for em after each step
            e_int[t:t + 1], e_bonus[t:t + 1], e_mod[t:t + 1] = T.replay_ngu(tw, A, frames, obs[t:t + 1], masks[t:t + 1],
                                                                            err[t:t + 1], warm[t:t + 1])
            assert _same(ems[16 * i + t][1].cpu().numpy(), tw.em), (i, t)
        assert _same(ro.int_rewards.cpu().numpy(), e_int), i
        assert _same(ro.episodic_bonus.cpu().numpy(), e_bonus) and _same(ro.ngu_modulator.cpu().numpy(), e_mod), i
        assert _same(ro.minv.cpu().numpy(), tw.minv) and _same(ro.count.cpu().numpy(), tw.count), i
        assert _same(ro.em.cpu().numpy(), tw.em) and (e_int > 0).any()
        any_mod = any_mod or bool((e_mod > 1).any())
    assert any_mod and tw.mod.seen["warm"] == 3 and tw.seen["reset"] >= 8


@pytest.mark.parametrize("cls_name", ["PPO", "PPO_NGU"])
def test_learn_one_iteration_logs_the_keys(monkeypatch, cls_name):
    import logger
    names, dumps = [], []
    real_configure, real_dump = logger.configure, logger.dump
    kw = dict(episodic=True) if cls_name == "PPO" else dict(rnd_start=4)
    alg = _make(cls_name, "KeyDoor-v0", episodic_kwargs=dict(ELL), **kw)
    monkeypatch.setattr(logger, "configure", lambda name, *a, **k: (names.append(name), real_configure(name, *a, **k)))
    monkeypatch.setattr(logger, "dump", lambda step=0: (dumps.append(logger.get_values()), real_dump(step)))
    alg.learn(total_timesteps=8 * 16, log_interval=1)
    torch.cuda.synchronize()
    assert names == ["PPO_Elliptical" if cls_name == "PPO" else "PPO_NGU_Elliptical"]
    assert len(dumps) == 1 and alg._n_updates == 1
    ro, log = alg.rollout, dumps[0]
    assert log["rollout/episodic_bonus"] == float(ro.episodic_bonus.mean().item()) > 0
    assert "rollout/episodic_dm" not in log
    assert ("rollout/ngu_modulator" in log) == (cls_name == "PPO_NGU")
    if cls_name == "PPO_NGU":
        assert log["rollout/ngu_modulator"] == float(ro.ngu_modulator.mean().item()) >= 1
        assert log["rollout/mean_int_reward"] == float(ro.int_rewards.mean().item()) > 0
    vals = logger.get_values()
    for k in ("train/policy_gradient_loss", "train/value_loss", "train/entropy_loss", "train/total_loss"):
        assert np.isfinite(vals[k]), k
    assert np.isfinite(alg.flat.data.detach().cpu().numpy()).all()


def test_refused_combinations_and_keywords(monkeypatch):
    import buffer
    import env as Env
    import ppo
    kd = dict(env_id="KeyDoor-v0", **CFG)
    ek = dict(episodic_kwargs=dict(ELL))
    with pytest.raises(NotImplementedError, match="sil"):
        ppo.PPO(episodic=True, sil=True, **ek, **kd)
    with pytest.raises(NotImplementedError, match="sim_hash"):
        ppo.PPO(episodic=True, sim_hash=True, **ek, **kd)
    with pytest.raises(NotImplementedError, match="PPO_RND"):
        ppo.PPO_RND(episodic=True, **kd)
    with pytest.raises(NotImplementedError, match="PPO_ICM"):
        ppo.PPO_ICM(episodic=True, **kd)
    with pytest.raises(NotImplementedError, match="uint8"):
        ppo.PPO(env_id="CartPole-v1", episodic=True, **ek, **CFG)
    with pytest.raises(NotImplementedError, match="uint8"):
        ppo.PPO_NGU(env_id="CartPole-v1", **ek, **CFG)
    for bad in (dict(k=3), dict(capacity=5), dict(decay=0.9), dict(mod_max=2.0)):
        with pytest.raises(TypeError, match="ridge, beta, frames"):
            ppo.PPO(episodic=True, episodic_kwargs=dict(ELL, **bad), **kd)
    for bad in (dict(beta=0.1), dict(k=3), dict(capacity=5)):
        with pytest.raises(TypeError, match="ridge, frames, mod_max"):
            ppo.PPO_NGU(episodic_kwargs=dict(ELL, **bad), **kd)
    for ridge in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="ridge"):
            ppo.PPO(episodic=True, episodic_kwargs=dict(ELL, ridge=ridge), **kd)
        with pytest.raises(ValueError, match="ridge"):
            ppo.PPO_NGU(episodic_kwargs=dict(ELL, ridge=ridge), **kd)
    with pytest.raises(ValueError, match="kind"):
        ppo.PPO(episodic=True, episodic_kwargs=dict(kind="e3b", nonsense=1), **kd)
    with pytest.raises(ValueError, match="kind"):
        ppo.PPO_NGU(episodic_kwargs=dict(kind="e3b", nonsense=1), **kd)
    with pytest.raises(ValueError, match="frames"):
        ppo.PPO(episodic=True, episodic_kwargs=dict(ELL, frames="first"), **kd)
    with pytest.raises(ValueError, match="mod_max"):
        ppo.PPO_NGU(episodic_kwargs=dict(ELL, mod_max=0.5), **kd)
    box = Env.Box((4, 84, 84), 0, 255, np.uint8)
    with pytest.raises(NotImplementedError, match="sim_hash"):
        buffer.RolloutStorage(4, 2, box, Env.Discrete(3), sim_hash=True, episodic=dict(ELL))
    with pytest.raises(NotImplementedError, match="uint8"):
        buffer.RolloutStorage(4, 2, Env.Box((4, 84, 84)), Env.Discrete(3), episodic=dict(ELL))
    st = buffer.RolloutStorage(4, 2, box, Env.Discrete(3), episodic=dict(ELL, ridge=4.0, beta=0.5))
    assert (st.epi_ridge, st.epi_beta) == (4.0, 0.5) and st.count.tolist() == [0, 0]
    assert _same(st.minv.cpu().numpy(), np.tile(np.eye(16) / 4.0, (2, 1, 1)))
    ist = buffer.IntrinsicStorage(4, 2, box, Env.Discrete(3), episodic=dict(ELL, ridge=8.0, mod_max=3.0))
    assert (ist.epi_ridge, ist.ngu_mod_max) == (8.0, 3.0) and ist.em.tolist() == list(G.EM_START)
    assert ist.ngu_modulator.shape == ist.rnd_err.shape == ist.int_rewards.shape == (4, 2)

    class Ctx:
        enabled, rank, world = True, 0, 2
    from dist import DistContext
    monkeypatch.setattr(DistContext, "current", staticmethod(lambda: Ctx()))
    with pytest.raises(NotImplementedError, match="process group"):
        ppo.PPO(episodic=True, **ek, **kd)
    with pytest.raises(NotImplementedError, match="process group"):
        ppo.PPO_NGU(**ek, **kd)


def test_default_kind_still_allocates_the_ring_and_matches_itself():
    """A PPO(episodic=True) without `kind` is the kNN bonus as before: mem and dm allocated, no minv, and two of
    them agree bit for bit over three rollouts."""
    a, b = (_make("PPO", "KeyDoor-v0", episodic=True) for _ in range(2))
    ro = a.rollout
    assert ro.epi_kind == "knn" and ro.mem.shape == (8, 5, 16) and ro.dm.shape == (2,) and not hasattr(ro, "minv")
    assert (ro.epi_capacity, ro.epi_k) == (5, 10) and ro.epi_coef == (0.99, 0.1, 1e-3, 8e-3, 1e-3, 8.0)
    for x, y in zip(_collect3(a), _collect3(b)):
        assert set(x) == set(y) and "mem" in x and "dm" in x
        for k in x:
            assert _same(x[k], y[k]), k
        assert (x["bonus"] > 0).any()
    n = _make("PPO_NGU", "KeyDoor-v0", rnd_start=4)
    assert n.rollout.epi_kind == "knn" and n.rollout.mem.shape == (8, 5, 16) and not hasattr(n.rollout, "minv")
