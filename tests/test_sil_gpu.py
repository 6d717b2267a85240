"""PPO(sil=True) on the device: the ppox_sil_* kernels, buffer.PrioritizedReplayBuffer and
sil_module.SilModule against tests/sil_twin.py (the definition).  Every tensor a
kernel writes is a view into a sentinel-filled allocation (tests/guarded.py)."""
import functools

import numpy as np
import pytest
import torch

import sil_twin as T
from guarded import Arena

pytestmark = pytest.mark.gpu

F64_INF = float("inf")


# ------------------------------------------------------------------------------------------ helpers
def dev_ring(ar, S, N, obs_shape=None, max_priority=1.0):
    P = T.capacity(S * N)
    ring = {"obs": None if obs_shape is None else ar.new((S, N) + obs_shape, torch.float32, init=0.0),
            "actions": ar.new((S, N), torch.int32, init=0), "log_probs": ar.new((S, N), torch.float32, init=0.0),
            "returns": ar.new((S, N), torch.float32, init=0.0), "dones": ar.new((S, N), torch.uint8, init=0),
            "state": ar.new((S, N), torch.uint8, init=0), "sum_tree": ar.new(2 * P, torch.float64, init=0.0),
            "min_tree": ar.new(2 * P, torch.float64, init=F64_INF)}
    mp = ar.new(1, torch.float64, init=max_priority)
    na = ar.new(1, torch.int64, init=-1)
    return ring, mp, na


def dev_trees(ar, s, m):
    """Device copies of two host trees (+ the state bytes of their leaves: active where sum > 0)."""
    P = len(s) // 2
    st = ar.new(2 * P, torch.float64, init=np.asarray(s))
    mt = ar.new(2 * P, torch.float64, init=np.asarray(m))
    state = ar.new(P, torch.uint8, init=(np.asarray(s)[P:] > 0).astype(np.uint8) * 2)
    return st, mt, state


def ulps(a, b):
    """Distance in float64 ulps between two positive arrays."""
    return np.abs(np.asarray(a, np.float64).view(np.int64) - np.asarray(b, np.float64).view(np.int64))


@functools.lru_cache(maxsize=None)
def rollouts(N, all_done):
    """Three appends of T = 4 steps for a ring of S = 6: env n follows pattern n % 5 —
    0: episodes that span appends (dones at global steps 5 and 10), 1: a done at the first step of
    every append, 2: a done at the last step of every append, 3: never done, 4: one episode longer
    than S (its only done at global step 9).  all_done: global step 6 is done in every env."""
    rs = np.random.RandomState(40 + N)
    Tn, n_app = 4, 3
    done = np.zeros((Tn * n_app, N), np.uint8)
    for n in range(N):
        k = n % 5
        if k == 0:
            done[[5, 10], n] = 1
        elif k == 1:
            done[[0, 4, 8], n] = 1
        elif k == 2:
            done[[3, 7, 11], n] = 1
        elif k == 4:
            done[9, n] = 1
    if all_done:
        done[6, :] = 1
    out = []
    for a in range(n_app):
        sl = slice(a * Tn, (a + 1) * Tn)
        out.append((rs.randint(0, 4, (Tn, N)).astype(np.int32), -rs.rand(Tn, N).astype(np.float32),
                    (rs.randn(Tn, N) * 2).astype(np.float32), done[sl].copy()))
    for arrs in out:
        for x in arrs:
            x.setflags(write=False)
    return tuple(out)


# ---------------------------------------------------------------------------------- returns and ring
@pytest.mark.parametrize("alpha", [1.0, 0.6])
@pytest.mark.parametrize("all_done", [False, True])
@pytest.mark.parametrize("N", [5, 64, 67])
def test_ring_returns_states_leaves(N, all_done, alpha):
    """N x S = 6, T = 4, three appends (the ring wraps): returns and states bitwise the twin's, pow leaves
    within 2 ulp (bitwise at alpha = 1), the rebuilt trees bitwise the twin's rebuild of the device's leaves."""
    import native
    S, gamma, mp0 = 6, 0.97, 2.5
    ar = Arena()
    ring, mp, na = dev_ring(ar, S, N, obs_shape=(3,), max_priority=mp0)
    tw = T.Ring(S, N, alpha=alpha, gamma=gamma)
    tw.max_priority = mp0
    exp_obs = np.zeros((S, N, 3), np.float32)
    head = 0
    rs = np.random.RandomState(7)
    for acts, lps, rews, dones in rollouts(N, all_done):
        obs = rs.randn(4, N, 3).astype(np.float32)
        for t in range(4):
            exp_obs[(head + t) % S] = obs[t]
        d = [torch.from_numpy(np.array(x)).cuda() for x in (obs, acts, lps, rews, dones)]
        native.sil_append(d[0], d[1], d[2], d[3], d[4], ring, head)
        head = (head + 4) % S
        native.sil_returns(ring, (head - 1) % S, gamma, alpha, mp)
        native.sil_tree_rebuild(ring["sum_tree"], ring["min_tree"], ring["state"], na)
        tw.step_rollout(acts, lps, rews, dones)
        ar.check()
        assert np.array_equal(ring["state"].cpu().numpy(), tw.state)
        assert np.array_equal(ring["returns"].cpu().numpy(), tw.returns)
        assert np.array_equal(ring["actions"].cpu().numpy(), tw.actions)
        assert np.array_equal(ring["log_probs"].cpu().numpy(), tw.log_probs)
        assert np.array_equal(ring["dones"].cpu().numpy(), tw.dones)
        assert np.array_equal(ring["obs"].cpu().numpy(), exp_obs)
        s, m = ring["sum_tree"].cpu().numpy(), ring["min_tree"].cpu().numpy()
        P = tw.P
        act = tw.sum_tree[P:] > 0
        assert np.array_equal(s[P:] > 0, act) and np.array_equal(np.isinf(m[P:]), ~act)
        assert np.array_equal(s[P:][~act], np.zeros((~act).sum()))
        assert np.array_equal(s[P:][act], m[P:][act])
        if alpha == 1.0:
            assert np.array_equal(s[P:], tw.sum_tree[P:])
        elif act.any():
            assert ulps(s[P:][act], tw.sum_tree[P:][act]).max() <= 2
        rs_, rm_ = T.rebuild(s[P:], m[P:])
        assert np.array_equal(s[1:], rs_[1:]) and np.array_equal(m[1:], rm_[1:])
        assert int(na.item()) == tw.n_active
    assert tw.n_active > 0 and (tw.state == T.PENDING).any()


def test_append_argument_checks():
    import native
    ar = Arena()
    ring, mp, na = dev_ring(ar, 6, 5)
    z = lambda dt: torch.zeros((7, 5), dtype=dt, device="cuda")  # noqa: E731
    with pytest.raises(native.NativeError, match="T <= S"):
        native.sil_append(None, z(torch.int32), z(torch.float32), z(torch.float32), z(torch.uint8), ring, 0)
    ar.check()


# -------------------------------------------------------------------------------------------- trees
@functools.lru_cache(maxsize=None)
def random_leaves(P, slots):
    rs = np.random.RandomState(P)
    s = np.zeros(P)
    live = rs.rand(slots) < 0.7
    s[:slots][live] = rs.rand(int(live.sum())) * 3 + 1e-3
    m = np.where(s > 0, s, np.inf)
    s.setflags(write=False)
    m.setflags(write=False)
    return s, m


@pytest.mark.parametrize("P,slots", [(32, 30), (65536, 65536), (1, 1), (2048, 1500)])
def test_tree_rebuild_bitwise(P, slots):
    import native
    ls, lm = random_leaves(P, slots)
    exp_s, exp_m = T.rebuild(ls, lm)
    junk_s, junk_m = exp_s.copy(), exp_m.copy()
    junk_s[1:P], junk_m[1:P] = -7.0, -7.0  # stale internal nodes
    ar = Arena()
    st, mt, state = dev_trees(ar, junk_s, junk_m)
    na = ar.new(1, torch.int64, init=-1)
    native.sil_tree_rebuild(st, mt, state[:slots], na)
    ar.check()
    assert np.array_equal(st.cpu().numpy()[1:], exp_s[1:]) and np.array_equal(mt.cpu().numpy()[1:], exp_m[1:])
    assert int(na.item()) == int((ls[:slots] > 0).sum())


@pytest.mark.parametrize("B", [1, 128, 1500])
@pytest.mark.parametrize("P", [32, 65536])
def test_priority_path_update_is_a_full_rebuild(P, B):
    """ppox_sil_update_priorities: leaves by last occurrence (bitwise at alpha = 1), max_priority, and the
    ancestors bitwise what a full rebuild of the same leaves gives."""
    import native
    slots = 30 if P == 32 else P
    ls, lm = random_leaves(P, slots)
    s0, m0 = T.rebuild(ls, lm)
    rs = np.random.RandomState(B)
    idx = rs.randint(0, slots, size=B).astype(np.int64)
    if B > 2:
        idx[-1] = idx[0]  # a repeated index whatever the draw
    pri = (rs.rand(B) * 6).astype(np.float32)
    pri[rs.rand(B) < 0.2] = 0.0  # clamped to 1e-6
    for alpha in (1.0, 0.6):
        ar = Arena()
        st, mt, state = dev_trees(ar, s0, m0)
        mp = ar.new(1, torch.float64, init=1.0)
        native.sil_update_priorities(torch.from_numpy(idx).cuda(), torch.from_numpy(pri).cuda(), alpha, st, mt, mp)
        ar.check()
        s, m = st.cpu().numpy(), mt.cpu().numpy()
        clamped = np.maximum(pri.astype(np.float64), 1e-6)
        assert float(mp.item()) == max(1.0, clamped.max())
        last = {int(i): p for i, p in zip(idx, clamped)}  # the last occurrence in batch order
        touched = np.array(sorted(last))
        exp = np.array([last[i] ** alpha for i in touched])
        print(f"P={P} B={B} alpha={alpha}: leaves off by at most {ulps(s[P + touched], exp).max()} ulp")
        if alpha == 1.0:
            assert np.array_equal(s[P + touched], exp)
        else:
            assert ulps(s[P + touched], exp).max() <= 2
        assert np.array_equal(s[P + touched], m[P + touched])
        rest = np.setdiff1d(np.arange(P), touched)
        assert np.array_equal(s[P + rest], s0[P + rest]) and np.array_equal(m[P + rest], m0[P + rest])
        rs_, rm_ = T.rebuild(s[P:], m[P:])
        assert np.array_equal(s[1:], rs_[1:]) and np.array_equal(m[1:], rm_[1:])
        # and the device's own rebuild of those leaves
        na = ar.new(1, torch.int64, init=-1)
        st2, mt2 = st.clone(), mt.clone()
        native.sil_tree_rebuild(st2, mt2, None, na)
        assert torch.equal(st2[1:], st[1:]) and torch.equal(mt2[1:], mt[1:]) and int(na.item()) == 0


# ----------------------------------------------------------------------------------------- sampling
def _sampling_trees(case):
    rs = np.random.RandomState(11)
    if case == "single":
        s = np.zeros(64)
        s[37] = 0.8
    elif case == "four":
        s = np.zeros(64)
        s[[3, 17, 18, 60]] = [0.5, 2.0, 1e-3, 1.25]
    elif case == "dense":
        s = rs.rand(4096) * 2 + 1e-3
    else:
        raise KeyError(case)
    return T.rebuild(s, np.where(s > 0, s, np.inf))


@pytest.mark.parametrize("beta", [0.0, 0.4, 1.0])
@pytest.mark.parametrize("case", ["single", "four", "dense"])
def test_sample_matches_twin(case, beta):
    import native
    s, m = _sampling_trees(case)
    P = len(s) // 2
    n = int((s[P:] > 0).sum())
    u = np.concatenate([np.random.RandomState(12).rand(1000), [0.0, 1.0 - 2.0 ** -53]])
    ar = Arena()
    st, mt, _ = dev_trees(ar, s, m)
    na = ar.new(1, torch.int64, init=n)
    idx = ar.new(len(u), torch.int64, init=-1)
    w = ar.new(len(u), torch.float32, init=-1.0)
    native.sil_sample(st, mt, na, torch.from_numpy(u).cuda(), beta, idx, w)
    ar.check()
    got = idx.cpu().numpy()
    assert np.array_equal(got, T.sample_indices(s, u))
    assert (s[P + got] > 0).all()  # every returned slot is active
    exp_w = T.weights(s, m, n, got, beta)
    if beta == 0.0:
        assert np.array_equal(w.cpu().numpy(), np.ones(len(u), np.float32))
    else:
        assert np.max(np.abs(w.cpu().numpy().astype(np.float64) - exp_w) / exp_w) <= 1e-6


def test_sample_guard_on_a_hand_built_node():
    """left <= mass and right == 0 at the root (as rounding of a parent sum can leave it): the plain
    descent ends on an empty leaf, the guarded one on the last active leaf."""
    import native
    s = np.array([0.0, 1.0, 0.5, 0.0, 0.25, 0.25, 0.0, 0.0])
    m = np.array([np.inf, 0.25, 0.25, np.inf, 0.25, 0.25, np.inf, np.inf])
    u = np.array([0.9, 0.5, 0.3, 0.0])
    assert T.sample_indices(s, u).tolist() == [1, 1, 1, 0]
    ar = Arena()
    st, mt, _ = dev_trees(ar, s, m)
    na = ar.new(1, torch.int64, init=2)
    idx, w = ar.new(4, torch.int64, init=-1), ar.new(4, torch.float32, init=-1.0)
    native.sil_sample(st, mt, na, torch.from_numpy(u).cuda(), 1.0, idx, w)
    ar.check()
    assert idx.cpu().numpy().tolist() == [1, 1, 1, 0]


# --------------------------------------------------------------------------------------------- loss
@functools.lru_cache(maxsize=None)
def loss_case(B, A):
    """Rows by b % 6: 0 delta < 0, 1 delta > 10, 2 rho > 1 + c, 3 rho < 1 - c, 4 saturated logits,
    5 plain; row 0 of B >= 7 batches has delta == 0 exactly."""
    rs = np.random.RandomState(100 * B + A)
    S, N = 41, 29  # 1,189 slots: every row of the largest batch has a slot of its own
    ring = {"actions": rs.randint(0, A, (S, N)).astype(np.int32), "log_probs": np.zeros((S, N), np.float32),
            "returns": (rs.randn(S, N) * 2).astype(np.float32)}
    idx = rs.permutation(S * N)[:B].astype(np.int64)
    logits = rs.randn(B, A).astype(np.float32)
    kind = np.arange(B) % 6
    logits[kind == 4] *= 60.0
    s, n = idx % S, idx // S
    R, act = ring["returns"][s, n], ring["actions"][s, n]
    values = (R - rs.rand(B).astype(np.float32) * 4 - np.float32(0.25)).astype(np.float32)  # 0.25 <= delta < 4.25
    values[kind == 0] = R[kind == 0] + rs.rand(int((kind == 0).sum())).astype(np.float32) + np.float32(0.5)
    values[kind == 1] = R[kind == 1] - np.float32(12.5)
    if B >= 7:
        values[6] = R[6]
    z = torch.from_numpy(logits)
    lp = torch.distributions.Categorical(torch.softmax(z, -1)).log_prob(torch.from_numpy(act).long()).numpy()
    old = lp + (rs.rand(B).astype(np.float32) - 0.5) * np.float32(0.2)       # rho within [0.9, 1.11]
    old[kind == 2] = lp[kind == 2] - np.float32(0.5)                         # rho = e^0.5
    old[kind == 3] = lp[kind == 3] + np.float32(0.5)                         # rho = e^-0.5
    ring["log_probs"][s, n] = old
    w = (rs.rand(B) * 0.9 + 0.1).astype(np.float32)
    ref = T.sil_loss(logits, values, act, old, R, w, 0.2, 0.01)
    return ring, idx, logits, values, w, ref, kind, S, N


@pytest.mark.parametrize("A", [1, 2, 4, 5, 18, 19, 33, 64])
@pytest.mark.parametrize("B", [1, 5, 128, 1027])
def test_sil_loss_vs_torch_autograd(B, A):
    """Losses <= 1e-5 relative, gradients <= 1e-4 relative against torch-CPU autograd (the project's loss
    tolerances); priorities bitwise clamp(delta, 0, 10)."""
    import native
    ring_h, idx, logits, values, w, ref, kind, S, N = loss_case(B, A)
    L, mean_a, dz_ref, dv_ref, a_ref, delta = ref
    ar = Arena()
    ring = {k: torch.from_numpy(v).cuda() for k, v in ring_h.items()}
    ring["state"] = torch.zeros((S, N), dtype=torch.uint8, device="cuda")
    dz = ar.new((B, A), torch.float32)
    dv, pri = ar.new(B, torch.float32), ar.new(B, torch.float32)
    partials = ar.new(native.LOSS_PARTIALS * 4, torch.float64)
    accum = ar.new(3, torch.float64, init=0.0)
    args = (torch.from_numpy(logits).cuda(), torch.from_numpy(values).cuda(), torch.from_numpy(idx).cuda(), ring,
            torch.from_numpy(w).cuda(), 0.2, 0.01, dz, dv, pri, partials, accum)
    native.sil_loss(*args)
    ar.check()
    acc = accum.cpu().numpy()
    print(f"B={B} A={A}: L {acc[0]:.9g} ref {L:.9g}; mean a {acc[1]:.9g} ref {mean_a:.9g}")
    np.testing.assert_allclose(acc[0], L, rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(acc[1], mean_a, rtol=1e-5, atol=1e-7)
    assert acc[2] == 1.0
    got_dz, got_dv = dz.cpu().numpy(), dv.cpu().numpy()
    np.testing.assert_allclose(got_dz, dz_ref, rtol=1e-4, atol=1e-5 * max(np.abs(dz_ref).max(), 1e-30))
    np.testing.assert_allclose(got_dv, dv_ref, rtol=1e-4, atol=1e-5 * max(np.abs(dv_ref).max(), 1e-30))
    s, n = idx % S, idx // S
    own_delta = ring_h["returns"][s, n] - values
    assert np.array_equal(pri.cpu().numpy(), np.clip(own_delta, np.float32(0), np.float32(10)))
    nonpos = own_delta <= 0
    assert not got_dz[nonpos].any() and not got_dv[nonpos].any()            # delta <= 0: exactly zero
    assert not got_dv[own_delta > 10].any()                                # delta > 10: no value gradient
    if B >= 128:
        assert nonpos.sum() > 1 and (own_delta > 10).any() and (own_delta == 0).any()
        plain = kind == 5
        assert np.abs(got_dv[plain]).max() > 0
        if A > 1:
            assert np.abs(got_dz[plain]).max() > 0
        # rho > 1 + c with a > 0: the clipped branch is the minimum, no policy gradient (entropy only)
        _, _, dz0, _, _, _ = T.sil_loss(logits, values, ring_h["actions"][s, n], ring_h["log_probs"][s, n],
                                        ring_h["returns"][s, n], w, 0.2, 0.0)
        assert not dz0[kind == 2].any() and (dz0[kind == 3].any() if A > 1 else not dz0.any())
    if A == 1:  # one action: softmax is the constant 1, no logit gradient on any row, exactly
        assert not got_dz.any() and not dz_ref.any()
    # a second call accumulates, bitwise the same contribution
    native.sil_loss(*args)
    acc2 = accum.cpu().numpy()
    assert acc2[2] == 2.0 and acc2[0] == acc[0] + acc[0] and acc2[1] == acc[1] + acc[1]


# --------------------------------------------------------------------------------------- end to end
def _weights(alg):
    return alg.flat.data.detach().cpu().numpy().copy()


def _run(env_id, sil, iters=2, **kw):
    import logger
    import ppo
    logger.configure("PPO_SIL" if sil else "PPO", env_id, quiet=True)
    np.random.seed(5)
    torch.manual_seed(5)
    alg = ppo.PPO(env_id=env_id, dynamics="real", sil=sil, n_envs=8, nstep=32, batch_size=64, n_epochs=1, quiet=True,
                  seed=3, **kw)
    rolls = []
    for _ in range(iters):
        alg.collect_samples()
        ro = alg.rollout
        rolls.append(tuple(x.cpu().numpy().copy() for x in (ro.actions, ro.log_probs, ro.rewards, ro.masks)))
        alg.train()
    torch.cuda.synchronize()
    return alg, rolls, dict(logger.get_values())


def _check_against_twin(alg, rolls):
    buf = alg.sil_module.buffer
    tw = T.Ring(buf.n_steps, buf.n_envs, alpha=buf.alpha, gamma=buf.gamma)
    for acts, lps, rews, dones in rolls:
        tw.append(acts, lps, rews, dones)
        tw.compute_returns()
    assert len(buf) == tw.n_active and tw.n_active > 100
    assert np.array_equal(buf.state.cpu().numpy(), tw.state)
    assert np.array_equal(buf.returns.cpu().numpy(), tw.returns)
    s, m = buf.buffer_sum.cpu().numpy(), buf.buffer_min.cpu().numpy()
    P = buf.capacity
    assert np.array_equal(s[P:] > 0, tw.sum_tree[P:] > 0)
    rs_, rm_ = T.rebuild(s[P:], m[P:])
    assert np.array_equal(s[1:], rs_[1:]) and np.array_equal(m[1:], rm_[1:])
    assert float(buf.max_priority.item()) >= 1.0


def test_ppo_sil_cartpole_end_to_end():
    """PPO(env_id="CartPole-v1", dynamics="real", sil=True, n_envs=8, nstep=32): two collect + train."""
    alg, rolls, logged = _run("CartPole-v1", True)
    assert alg.sil_module.buffer.n_steps == 6250 and alg.sil_module.buffer.capacity == 65536  # ceil(50000 / 8)
    _check_against_twin(alg, rolls)
    assert np.isfinite(logged["train/sil_loss"]) and np.isfinite(logged["rollout/mean_sil_advantage"])
    assert logged["rollout/mean_sil_advantage"] >= 0
    w_sil = _weights(alg)
    assert np.isfinite(w_sil).all()
    base, _, logged0 = _run("CartPole-v1", False)
    assert base.sil_module is None and "train/sil_loss" not in logged0
    assert not np.array_equal(w_sil, _weights(base))
    # the same seed again: SIL is deterministic run to run
    again, _, _ = _run("CartPole-v1", True)
    assert np.array_equal(w_sil, _weights(again))


def test_ppo_sil_catch_frames_stay_in_the_ring():
    """Catch-v0: uint8 frame stacks; the SIL minibatch is read in place (convs.RolloutRows over the ring)."""
    import convs
    alg, rolls, logged = _run("Catch-v0", True, sil_kwargs=dict(size=2048, batch=96, epochs=2))
    buf = alg.sil_module.buffer
    assert buf.n_steps == 256 and buf.observations.dtype == torch.uint8
    assert tuple(buf.observations.shape) == (256, 8, 4, 84, 84)
    _check_against_twin(alg, rolls)
    rows = alg._train_obs(buf, torch.zeros(4, dtype=torch.int64, device="cuda"))
    assert isinstance(rows, convs.RolloutRows) and rows.T == 256 and rows.frames.data_ptr() == buf.observations.data_ptr()
    # the ring's frames are the rollouts' (two appends of 32 steps from step 0)
    assert torch.equal(buf.observations[32:64], alg.rollout.observations)
    assert np.isfinite(logged["train/sil_loss"]) and "rollout/mean_sil_advantage" in logged
    assert np.isfinite(_weights(alg)).all()


def test_sil_refusals(monkeypatch):
    import ppo
    from dist import DistContext
    with pytest.raises(NotImplementedError, match="Discrete"):
        ppo.PPO(env_id="Pendulum-v1", dynamics="real", sil=True, n_envs=4, nstep=8, quiet=True)
    with pytest.raises(NotImplementedError, match="sim_hash"):
        ppo.PPO(env_id="CartPole-v1", dynamics="real", sil=True, sim_hash=True, n_envs=4, nstep=8, quiet=True)
    with pytest.raises(TypeError, match="sil_kwargs"):
        ppo.PPO(env_id="CartPole-v1", dynamics="real", sil=True, n_envs=4, nstep=8, quiet=True,
                sil_kwargs=dict(gamma=0.5))
    monkeypatch.setattr(ppo.DistContext, "current", classmethod(lambda cls: DistContext(0, 2)))
    with pytest.raises(NotImplementedError, match="process group"):
        ppo.PPO(env_id="CartPole-v1", dynamics="real", sil=True, n_envs=4, nstep=8, quiet=True)
