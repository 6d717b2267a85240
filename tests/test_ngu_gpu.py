"""PPO_NGU on the device (ppox_ngu_reward of csrc/episodic.hip, IntrinsicStorage.ngu, ppo.PPO_NGU) against the
numpy twin (tests/ngu_twin.py).  The embeddings and distances are integers and every float64 operation is done in
a stated order, so every comparison is bit for bit."""
import functools

import numpy as np
import pytest
import torch

import episodic_twin as E
import ngu_twin as T
import simhash_px_twin as H

pytestmark = pytest.mark.gpu

FRAME = 84 * 84
GUARD = -7.0


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def _knn_state(N, L, K):
    d = "cuda"
    return dict(mem=torch.zeros((N, L, 16), dtype=torch.int32, device=d),
                count=torch.zeros(N, dtype=torch.int32, device=d),
                dm=torch.zeros(2, dtype=torch.float64, device=d),
                dk=torch.full((N, K), -1.0, dtype=torch.float64, device=d),
                kfound=torch.full((N,), -1, dtype=torch.int32, device=d),
                mk=torch.full((N,), -1.0, dtype=torch.float64, device=d))


# ----------------------------------------------------------------------------------------------------- kernel
@pytest.mark.parametrize("case", T.CASES, ids=T.case_id)
def test_ngu_reward_equals_twin_at_every_step(case):
    """3 L + 2 steps of knn -> ngu_reward against the twin: mem, count, dm, em, dk (masked by kfound), kfound, mk,
    bonus, modulator and int_rewards after every step; the rows between the three outputs keep their fill."""
    import native
    N, L, K = case["N"], case["L"], case["K"]
    tw, emb, done, err, warm = T.make(case)
    s = _knn_state(N, L, K)
    em = torch.tensor(tw.em.tolist(), dtype=torch.float64, device="cuda")
    out = torch.full((7, N), GUARD, device="cuda")         # guard, int_rewards, guard, bonus, guard, modulator, guard
    emb_d, done_d, err_d = (torch.from_numpy(a).cuda() for a in (emb, done, err))
    for t in range(len(emb)):
        e_dk, e_kf, e_mk = tw.knn_step(emb[t], done[t])
        em_before = tw.em.copy()
        e_int, e_bonus, e_mod = tw.ngu_step(e_dk, e_kf, e_mk, None if t < warm else err[t])
        native.episodic_knn(emb_d[t], done_d[t], N, L, K, s["mem"], s["count"], s["dk"], s["kfound"], s["mk"])
        native.ngu_reward(s["dk"], s["kfound"], s["mk"], None if t < warm else err_d[t], N, K, s["dm"], em, tw.decay,
                          tw.eps, tw.xi, tw.c, tw.smax, tw.mod_max, out[1], out[3], out[5])
        assert _same(s["kfound"].cpu().numpy(), e_kf), t
        live = np.arange(K)[None, :] < e_kf[:, None]
        assert _same(np.where(live, s["dk"].cpu().numpy(), 0.0), e_dk), t
        assert _same(s["mk"].cpu().numpy(), e_mk), t
        assert _same(s["mem"].cpu().numpy(), tw.mem) and _same(s["count"].cpu().numpy(), tw.count), t
        assert _same(s["dm"].cpu().numpy(), tw.dm), t
        assert _same(em.cpu().numpy(), tw.em), (t, em.cpu().numpy(), tw.em)
        if t < warm:
            assert _same(tw.em, em_before)
        o = out.cpu().numpy()
        assert _same(o[3], e_bonus), t
        assert _same(o[5], e_mod), t
        assert _same(o[1], e_int), t
        assert (o[0::2] == GUARD).all(), t
    missing = [b for b in E.case_branches(case) if tw.seen[b] == 0]
    assert not missing, (missing, tw.seen)
    assert tw.seen["warm"] == warm
    if case["err"] == "const":
        assert tw.seen["sigma0"] == len(emb) * N
    else:
        assert tw.seen["lo"] >= 1 and tw.seen["mid"] >= 1
        assert tw.seen["hi"] >= 1 or case["err"] == "warm3" or N < 64


@pytest.mark.parametrize("case", T.CASES, ids=T.case_id)
def test_episodic_reward_is_unchanged_by_the_shared_helpers(case):
    """The same cases (N above 1,024 included: several envs per thread in the pair tree) through
    ppox_episodic_reward == Episodic.reward_step: dm, bonus and rewards after every step."""
    import native
    N, L, K = case["N"], case["L"], case["K"]
    emb, done, rew = E.case_inputs(case)
    tw = E.Episodic(N, L, K, smax=case["smax"])
    dm = torch.zeros(2, dtype=torch.float64, device="cuda")
    bonus = torch.full((N,), -1.0, device="cuda")
    rew_d = torch.from_numpy(rew).cuda()
    for t in range(len(emb)):
        e_dk, e_kf, e_mk = tw.knn_step(emb[t], done[t])
        e_rew, e_bonus = tw.reward_step(e_dk, e_kf, e_mk, rew[t])
        dk, kf, mk = (torch.from_numpy(a).cuda() for a in (e_dk, e_kf, e_mk))
        native.episodic_reward(dk, kf, mk, N, K, dm, tw.decay, tw.beta, tw.eps, tw.xi, tw.c, tw.smax, rew_d[t], bonus)
        assert _same(dm.cpu().numpy(), tw.dm), t
        assert _same(bonus.cpu().numpy(), e_bonus) and _same(rew_d[t].cpu().numpy(), e_rew), t


def test_argument_checks_come_before_any_launch():
    import native
    lib = native.load()
    x = torch.zeros(64, dtype=torch.float64, device="cuda")
    p = x.data_ptr()
    coef = (.99, 1e-3, 8e-3, 1e-3, 8.)

    def call(dk=p, kf=p, mk=p, err=p, N=4, K=4, dm=p, em=p, mod_max=5., ir=p, bonus=p, mod=p):
        return lib.ppox_ngu_reward(dk, kf, mk, err, N, K, dm, em, *coef, mod_max, ir, bonus, mod, None)
    for name in ("dk", "kf", "mk", "dm", "em", "ir", "bonus", "mod"):
        assert call(**{name: None}) == -1000, name
        assert b"ppox_ngu_reward: null pointer" in lib.ppox_last_error()
    for kw in (dict(N=0), dict(N=2 ** 31), dict(K=0), dict(K=17), dict(mod_max=0.5), dict(mod_max=float("nan"))):
        assert call(**kw) == -1000, kw
        assert b"ppox_ngu_reward" in lib.ppox_last_error() and b"null" not in lib.ppox_last_error()
    assert b"mod_max" in lib.ppox_last_error()
    torch.cuda.synchronize()
    assert (x == 0).all()                                     # nothing was launched
    # a null err is accepted: one env without neighbours, modulator 1, em untouched
    kf = torch.zeros(1, dtype=torch.int32, device="cuda")
    em = torch.tensor(T.EM_START, dtype=torch.float64, device="cuda")
    out = torch.full((3,), GUARD, device="cuda")
    assert lib.ppox_ngu_reward(p, kf.data_ptr(), p, None, 1, 4, p, em.data_ptr(), *coef, 1.0, out[0:].data_ptr(),
                               out[1:].data_ptr(), out[2:].data_ptr(), None) == 0
    assert out.tolist() == [0.0, 0.0, 1.0] and em.tolist() == list(T.EM_START)


# -------------------------------------------------------------------------------------------------- algorithm
CFG = dict(n_envs=8, nstep=16, batch_size=64, n_epochs=1, quiet=True, dynamics="real", rnd_start=4)
ENVS = {"KeyDoor-v0": dict(seed=11, max_len=5), "Catch-v0": dict(seed=3, max_len=None)}


def _make(cls_name, env_id, **kw):
    import env as Env
    import logger
    import ppo
    logger.configure(cls_name, env_id, quiet=True)
    spec = ENVS[env_id]
    np.random.seed(0)
    torch.manual_seed(0)
    if spec["max_len"] is not None:
        kw["env"] = Env.make_env(env_id, n_envs=8, seed=spec["seed"], dynamics="real", max_len=spec["max_len"])
    return getattr(ppo, cls_name)(env_id=env_id, seed=spec["seed"], **CFG, **kw)


@functools.lru_cache(maxsize=None)
def twin_matrix(D, seed):
    A = H.matrix(D, seed)
    A.setflags(write=False)
    return A


_SHARED = ("rewards", "masks", "actions", "values", "obs_slots")


@pytest.mark.parametrize("env_id", list(ENVS))
def test_ppo_ngu_equals_twin_replay_over_three_collects(env_id):
    """8 envs x 16 steps, three collects without train(): episodes end inside the rollouts and the state crosses
    two rollout boundaries.  The first three steps run before rnd_start (modulator 1, em at its start)."""
    ngu = _make("PPO_NGU", env_id, episodic_kwargs=dict(k=3))
    rnd = _make("PPO_RND", env_id)
    ro = ngu.rollout
    L = ENVS[env_id]["max_len"] or 256
    assert (ro.epi_capacity, ro.epi_k, ro.epi_frames, ro.epi_D, ro.ngu_mod_max) == (L, 3, "last", FRAME, 5.0)
    assert ro.epi_seed == ENVS[env_id]["seed"] and ro.em.tolist() == list(T.EM_START)
    assert not hasattr(rnd.rollout, "em") and not rnd.rollout.do_episodic
    ems, real_ngu = [], ro.ngu

    def recording_ngu(obs, dones, err, t=None):
        out = real_ngu(obs, dones, err, t)
        ems.append((err is None, ro.em.clone()))
        return out
    ro.ngu = recording_ngu
    A = twin_matrix(FRAME, ro.epi_seed)
    tw = T.Ngu(8, L, K=3)
    any_mod = False
    for i in range(3):
        ngu.collect_samples()
        rnd.collect_samples()
        for k in _SHARED:                                   # the bonus leaves the env's stream as it is
            assert _same(getattr(ro, k).cpu().numpy(), getattr(rnd.rollout, k).cpu().numpy()), (i, k)
        warm = np.array([w for w, _ in ems[16 * i:]])
        assert warm.tolist() == ([True] * 3 + [False] * 13 if i == 0 else [False] * 16)
        obs, masks = ro.obs_slots.cpu().numpy(), ro.masks.cpu().numpy()
        assert masks.sum() > 0
        state = []
        e_int = np.empty((16, 8), np.float32)
        e_bonus, e_mod = np.empty_like(e_int), np.empty_like(e_int)
        err = ro.rnd_err.cpu().numpy()
        for t in range(16):                                 # T.replay, one step at a time for em after each step
            e_int[t:t + 1], e_bonus[t:t + 1], e_mod[t:t + 1] = T.replay(tw, A, "last", obs[t:t + 1], masks[t:t + 1],
                                                                       err[t:t + 1], warm[t:t + 1])
            state.append(tw.em.copy())
            assert _same(ems[16 * i + t][1].cpu().numpy(), tw.em), (i, t)
            if warm[t]:
                assert tw.em.tolist() == list(T.EM_START) and (e_mod[t] == 1).all()
        assert _same(ro.int_rewards.cpu().numpy(), e_int), i
        assert _same(ro.episodic_bonus.cpu().numpy(), e_bonus) and _same(ro.ngu_modulator.cpu().numpy(), e_mod), i
        assert _same(ro.mem.cpu().numpy(), tw.mem) and _same(ro.count.cpu().numpy(), tw.count), i
        assert _same(ro.dm.cpu().numpy(), tw.dm) and _same(ro.em.cpu().numpy(), tw.em), i
        assert (e_int > 0).any()
        any_mod = any_mod or bool((e_mod > 1).any())
        if i:
            assert (err > 0).any() and np.isfinite(err).all()
    assert any_mod and tw.seen["warm"] == 3 and tw.seen["reset"] >= 8 and tw.seen["mid"] + tw.seen["hi"] > 0


@pytest.mark.parametrize("coef", [1.0, 0.3])
def test_learn_one_iteration_logs_and_weights_the_intrinsic_advantage(monkeypatch, coef):
    import logger
    import native
    names, dumps, raw, used = [], [], [], []
    real_configure, real_dump, real_stats = logger.configure, logger.dump, native.minibatch_adv_stats
    alg = _make("PPO_NGU", "KeyDoor-v0", int_adv_coef=coef)
    assert alg.int_adv_coef == coef and alg.rollout.epi_capacity == 5 and alg.rollout.epi_k == 10
    monkeypatch.setattr(logger, "configure", lambda name, *a, **k: (names.append(name), real_configure(name, *a, **k)))
    monkeypatch.setattr(logger, "dump", lambda step=0: (dumps.append(logger.get_values()), real_dump(step)))

    def stats_spy(adv, iadv, perm, total, bs, T_, N_, stats, *a, **k):
        real_stats(adv, iadv, perm, total, bs, T_, N_, stats, *a, **k)
        raw.append(stats.clone())
    monkeypatch.setattr(native, "minibatch_adv_stats", stats_spy)
    real_loss = alg._loss_grads

    def loss_spy(od, vd, ivd, idx, roll, stats, *a, **k):
        used.append(stats.clone())
        return real_loss(od, vd, ivd, idx, roll, stats, *a, **k)
    alg._loss_grads = loss_spy
    alg.learn(total_timesteps=8 * 16, log_interval=1)
    torch.cuda.synchronize()
    assert names == ["PPO_NGU"] and len(dumps) == 1 and alg._n_updates == 1
    ro, log = alg.rollout, dumps[0]
    assert log["rollout/episodic_bonus"] == float(ro.episodic_bonus.mean().item()) > 0
    assert log["rollout/episodic_dm"] == float(ro.dm[0].item()) > 0
    assert log["rollout/ngu_modulator"] == float(ro.ngu_modulator.mean().item()) >= 1
    assert log["rollout/mean_int_reward"] == float(ro.int_rewards.mean().item()) > 0
    vals = logger.get_values()
    for k in ("train/policy_gradient_loss", "train/value_loss", "train/entropy_loss", "train/total_loss",
              "train/intrinsic_loss"):
        assert np.isfinite(vals[k]), k
    assert np.isfinite(alg.flat.data.detach().cpu().numpy()).all()
    assert np.isfinite(alg.rnd_flat.data.detach().cpu().numpy()).all()
    assert len(raw) == 1 and len(used) == 2                  # 128 rows in minibatches of 64, one epoch
    raw, used = raw[0].cpu().numpy(), torch.stack(used).cpu().numpy()
    assert raw.shape == used.shape == (2, 4) and (raw[:, 3] > 0).all()
    assert _same(used[:, :3], raw[:, :3])
    if coef == 1.0:
        assert _same(used, raw)
    else:
        assert (used[:, 3] != raw[:, 3]).all()
        # (std' + 1e-8) = (std + 1e-8) / w: the kernels' quotient is w times the normalised advantage
        assert np.allclose(used[:, 3] + 1e-8, (raw[:, 3] + 1e-8) / coef, rtol=1e-12, atol=0)


def test_refusals(monkeypatch):
    import buffer
    import env as Env
    import ppo
    import algorithms
    assert algorithms.PPO_NGU is ppo.PPO_NGU and issubclass(ppo.PPO_NGU, ppo.PPO_RND)
    kd = dict(env_id="KeyDoor-v0", **CFG)
    with pytest.raises(NotImplementedError, match="uint8"):
        ppo.PPO_NGU(env_id="CartPole-v1", **CFG)
    with pytest.raises(TypeError, match="capacity.*frames.*mod_max"):
        ppo.PPO_NGU(episodic_kwargs=dict(beta=0.1), **kd)
    with pytest.raises(TypeError, match="capacity.*frames.*mod_max"):
        ppo.PPO_NGU(episodic_kwargs=dict(kk=3), **kd)
    with pytest.raises(ValueError, match="int_adv_coef"):
        ppo.PPO_NGU(int_adv_coef=0.0, **kd)
    with pytest.raises(NotImplementedError, match="NGU's product"):
        ppo.PPO_RND(episodic=True, **kd)
    box = Env.Box((4, 84, 84), 0, 255, np.uint8)
    st = buffer.IntrinsicStorage(4, 2, box, Env.Discrete(3), episodic=dict(capacity=7, mod_max=3.0))
    assert st.mem.shape == (2, 7, 16) and st.ngu_mod_max == 3.0 and st.em.tolist() == list(T.EM_START)
    assert st.ngu_modulator.shape == st.rnd_err.shape == st.int_rewards.shape == (4, 2)
    plain = buffer.IntrinsicStorage(4, 2, box, Env.Discrete(3))
    assert not plain.do_episodic and not hasattr(plain, "em") and not hasattr(plain, "ngu_modulator")

    class Ctx:
        enabled, rank, world = True, 0, 2
    from dist import DistContext
    monkeypatch.setattr(DistContext, "current", staticmethod(lambda: Ctx()))
    with pytest.raises(NotImplementedError, match="process group"):
        ppo.PPO_NGU(**kd)


def test_storage_add_pays_the_product_on_the_intrinsic_stream():
    """IntrinsicStorage.add with the episodic state: int_reward is the raw error (None: warm-up), the rewards stay
    as given, and episodic() is never called."""
    import buffer
    import env as Env
    box = Env.Box((4, 84, 84), 0, 255, np.uint8)
    st = buffer.IntrinsicStorage(3, 2, box, Env.Discrete(3), episodic=dict(capacity=4, k=2), hash_seed=5)
    st.episodic = None                                          # calling it would raise
    A = twin_matrix(FRAME, 5)
    tw = T.Ngu(2, 4, K=2)
    rs = np.random.RandomState(0)
    obs = rs.randint(0, 256, (3, 2, 4, 84, 84)).astype(np.uint8)
    obs[2, 0] = obs[0, 0]                                       # a revisited frame
    rew = rs.randn(3, 2).astype(np.float32)
    err = np.array([[0, 0], [0.5, 2.0], [4.0, 0.25]], np.float32)
    masks = np.zeros((3, 2), np.uint8)
    for t in range(3):
        st.add(obs[t], np.zeros(2, np.int32), rew[t], None if t == 0 else err[t], np.zeros(2, np.float32),
               np.zeros(2, np.float32), masks[t], np.zeros(2, np.float32))
    e_int, e_bonus, e_mod = T.replay(tw, A, "last", obs, masks, err, np.array([True, False, False]))
    assert st.full and _same(st.rewards.cpu().numpy(), rew)
    assert _same(st.int_rewards.cpu().numpy(), e_int) and _same(st.episodic_bonus.cpu().numpy(), e_bonus)
    assert _same(st.ngu_modulator.cpu().numpy(), e_mod) and _same(st.em.cpu().numpy(), tw.em)
    assert _same(st.rnd_err.cpu().numpy()[1:], err[1:]) and (e_int[1:] > 0).all()
    plain = buffer.IntrinsicStorage(3, 2, box, Env.Discrete(3))                 # without it: int_rewards as given
    plain.add(obs[0], np.zeros(2, np.int32), rew[0], err[1], np.zeros(2, np.float32), np.zeros(2, np.float32),
              masks[0], np.zeros(2, np.float32))
    assert _same(plain.int_rewards.cpu().numpy()[0], err[1]) and _same(plain.rewards.cpu().numpy()[0], rew[0])
