"""PPO_NGU's numpy twin (tests/ngu_twin.py) on the CPU: its episodic part against the episodic twin bit for bit,
its Chan merge against util.RunningMeanStd, the warm-up, the storage's keyword checks, and that every case the GPU
file drives reaches the modulator's branches it is there for (so the seeds are settled here, without a GPU)."""
import math

import numpy as np
import pytest

import episodic_twin as E
import ngu_twin as T


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


def _run(case):
    tw, emb, done, err, warm = T.make(case)
    outs = []
    for t in range(len(emb)):
        dk, kf, mk = tw.knn_step(emb[t], done[t])
        outs.append(tw.ngu_step(dk, kf, mk, None if t < warm else err[t]))
    return tw, outs, err, warm


@pytest.mark.parametrize("case", T.CASES, ids=T.case_id)
def test_cases_reach_the_modulator_branches(case):
    tw, outs, err, warm = _run(case)
    S, N, kind = len(outs), case["N"], case["err"]
    seen = tw.seen
    assert seen["warm"] == (3 if kind == "warm3" else 0) == warm
    assert seen["sigma0"] + seen["lo"] + seen["mid"] + seen["hi"] == (S - warm) * N
    if kind == "const":
        assert seen["sigma0"] == S * N and tw.em.tolist() == [0.25, 0.0, float(S * N)]
        assert all((o[2] == 1).all() for o in outs)
    else:
        assert seen["sigma0"] == 0 and seen["lo"] >= 1 and seen["mid"] >= 1, seen
        if kind in ("outlier", "lognormal") and N >= 64:
            assert seen["hi"] >= 1, seen
    for int_rew, bonus, mod in outs:
        assert int_rew.dtype == bonus.dtype == mod.dtype == np.float32
        assert (mod >= 1).all() and (mod <= T.MOD_MAX).all() and np.isfinite(int_rew).all()
    missing = [b for b in E.case_branches(case) if seen[b] == 0]          # the episodic branches, as before
    assert not missing, (missing, seen)


def test_cases_are_the_episodic_ones_with_rotating_error_kinds_and_two_wide_ones():
    assert len(T.CASES) == len(E.CASES) + 2 == 22
    for i, (c, e) in enumerate(zip(T.CASES, E.CASES)):
        assert {k: v for k, v in c.items() if k != "err"} == e and c["err"] == T.KINDS[i % 4]
    assert [(c["N"], c["L"], c["K"], c["kind"], c["done"], c["err"]) for c in T.CASES[-2:]] == \
        [(1025, 2, 3, "small", "bern", "lognormal"), (2500, 2, 3, "small", "bern", "lognormal")]
    for c in T.CASES:
        err, warm, em = T.case_errors(c)
        assert err.shape == (3 * c["L"] + 2, c["N"]) and err.dtype == np.float32 and np.isfinite(err).all()
        if c["err"] == "outlier":
            assert (err[1::2, 0] == 50.0).all() and (err[0::2, 0] == np.float32(1e-3)).all()
        assert em == ((0.0, 0.0, 0.0) if c["err"] == "const" else T.EM_START)


@pytest.mark.parametrize("case", T.CASES[:8], ids=T.case_id)
def test_modulator_one_gives_the_episodic_twins_bonus_bit_for_bit(case):
    """err=None at every step: int_rewards == bonus == Episodic.reward_step's bonus, dm the same, em untouched."""
    emb, done, rew = E.case_inputs(case)
    ref = E.Episodic(case["N"], case["L"], case["K"], smax=case["smax"])
    tw = T.Ngu(case["N"], case["L"], case["K"], smax=case["smax"])
    for t in range(len(emb)):
        dk, kf, mk = ref.knn_step(emb[t], done[t])
        dk2, kf2, mk2 = tw.knn_step(emb[t], done[t])
        assert np.array_equal(dk, dk2) and np.array_equal(kf, kf2) and np.array_equal(mk, mk2)
        _, e_bonus = ref.reward_step(dk, kf, mk, rew[t])
        int_rew, bonus, mod = tw.ngu_step(dk, kf, mk, None)
        assert np.array_equal(_bits(bonus), _bits(e_bonus)) and np.array_equal(_bits(int_rew), _bits(e_bonus)), t
        assert (mod == 1).all() and np.array_equal(_bits(tw.dm), _bits(ref.dm))
    assert tw.em.tolist() == list(T.EM_START) and tw.seen["warm"] == len(emb)


def test_err_none_leaves_em_untouched_between_updates():
    tw = T.Ngu(4, 3, K=2)
    e = np.array([0.5, 1.0, 2.0, 4.0], np.float32)
    tw.modulator_step(e)
    em = tw.em.copy()
    assert not np.array_equal(em, np.array(T.EM_START))
    assert (tw.modulator_step(None) == 1).all() and np.array_equal(_bits(tw.em), _bits(em))
    tw.modulator_step(e)
    assert tw.em[2] == (1e-4 + 4.0) + 4.0 and not np.array_equal(tw.em, em)


@pytest.mark.parametrize("N", [1, 3, 64, 257, 2500])
def test_chan_merge_equals_running_mean_std(N):
    """The twin's em against util.RunningMeanStd.update_from_moments fed the same batches' numpy moments: the
    batch sums are in another order (tree against numpy's pairwise), so 1e-12 relative, not bitwise."""
    from util import RunningMeanStd
    rs = np.random.RandomState(N)
    tw = T.Ngu(N, 2, K=1)
    rms = RunningMeanStd(device="cpu")
    for _ in range(6):
        e = np.exp(2.0 * rs.randn(N)).astype(np.float32)
        tw.modulator_step(e)
        e64 = e.astype(np.float64)
        rms.update_from_moments(e64.mean(), e64.var(), N)
        got = tw.em
        exp = np.array([float(rms.mean), float(rms.var), float(rms.count)])
        assert np.allclose(got, exp, rtol=1e-12, atol=0), (got, exp)


def test_modulator_on_hand_values():
    tw = T.Ngu(4, 2, K=1, mod_max=2.0, em=(0.0, 0.0, 0.0))
    e = np.array([1.0, 3.0, 5.0, 7.0], np.float32)               # mean 4, variance 5, exact
    mod = tw.modulator_step(e)
    assert tw.em.tolist() == [4.0, 5.0, 4.0]
    s = math.sqrt(5.0)
    assert mod.tolist() == [1.0, 1.0, 1.0 + 1.0 / s, 2.0]        # a = 1 - 3/s, 1 - 1/s, 1 + 1/s, 1 + 3/s > 2
    assert (tw.seen["lo"], tw.seen["mid"], tw.seen["hi"], tw.seen["sigma0"]) == (2, 1, 1, 0)
    r = np.array([0.5, 0.25, 0.125, 1.0])
    tw2 = T.Ngu(4, 2, K=1, mod_max=2.0, em=(4.0, 5.0, 4.0))
    tw2.r_step = lambda dk, kf, mk: r
    tw2.modulator_step = lambda err: mod
    int_rew, bonus, m32 = tw2.ngu_step(None, None, None, e)
    assert int_rew.tolist() == [0.5, 0.25, np.float32(0.125 * (1.0 + 1.0 / s)), 2.0]
    assert bonus.tolist() == r.tolist() and m32.tolist() == mod.astype(np.float32).tolist()


def test_storage_refuses_beta_and_unknown_keys_before_it_allocates():
    import buffer
    import env as Env
    box = Env.Box((4, 84, 84), 0, 255, np.uint8)
    assert set(buffer.NGU_DEFAULTS) == set(buffer.EPISODIC_DEFAULTS) - {"beta"} | {"mod_max"} == set(T.DEFAULTS)
    assert buffer.NGU_DEFAULTS == T.DEFAULTS and buffer.NGU_DEFAULTS["mod_max"] == 5.0
    for bad in (dict(beta=0.1), dict(kk=3), dict(k=3, modmax=2.0)):
        with pytest.raises(TypeError, match="capacity.*frames.*mod_max"):
            buffer.IntrinsicStorage(4, 2, box, Env.Discrete(3), device="cpu", episodic=bad)
    with pytest.raises(ValueError, match="mod_max"):
        buffer.IntrinsicStorage(4, 2, box, Env.Discrete(3), device="cpu", episodic=dict(mod_max=0.5))
