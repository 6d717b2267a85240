"""The elliptical bonus's numpy twin (tests/elliptical_twin.py) on the CPU: against a direct
inverse, its invariants, the branches its cases are there for, hand-written values, and the keyword and argument
checks that run before any launch."""
import functools
import os

import numpy as np
import pytest

import elliptical_twin as T
import episodic_twin as E

CASES = T.cpu_cases()
PARITY = [c for c in CASES if c is not T.CLAMP_CASE]
# 100 x the worst relative difference measured per group (the docstring of the test below)
BOUND = {("small", 1.0): 1.2e-13, ("identical", 1.0): 9.6e-7, ("extreme", 2.0 ** 40): 2.4e-9,
         ("extreme", 2.0 ** 54): 2.3e-13}


@functools.lru_cache(maxsize=None)
def run(i):
    """Case i through the twin once, shared by the tests: per step b_raw, pay, the direct inverse's b, and whether
    M was finite and bitwise symmetric; then the branch counts."""
    c = CASES[i]
    emb, done, rew = E.case_inputs(c)
    tw = T.Elliptical(c["N"], c["ridge"])
    C = np.tile(np.eye(16) * c["ridge"], (c["N"], 1, 1))
    steps = []
    for t in range(len(emb)):
        phi = emb[t].astype(np.float64)
        direct = None
        if c is not T.CLAMP_CASE:                          # (at ridge 1 the extreme C is singular in float64)
            direct = np.einsum("ni,nij,nj->n", phi, np.linalg.inv(C), phi)
        pay = tw.bonus_step(emb[t], done[t])
        steps.append(dict(b_raw=tw.b_raw.copy(), pay=pay, direct=direct, finite=bool(np.isfinite(tw.minv).all()),
                          symmetric=np.array_equal(tw.minv, tw.minv.transpose(0, 2, 1))))
        C = C + phi[:, :, None] * phi[:, None, :]
        C[done[t] != 0] = np.eye(16) * c["ridge"]
    return steps, dict(tw.seen), done


@pytest.mark.parametrize("i", [CASES.index(c) for c in PARITY], ids=[T.case_id(c) for c in PARITY])
def test_b_raw_equals_the_direct_inverse(i):
    """The twin's b_raw against phi' inv(ridge I + sum phi phi') phi from np.linalg.inv, over episodic_twin.CASES.
    Worst relative differences measured with this twin (|twin - direct| / |direct|, absolute where direct is 0):
      small      ridge 1     1.12e-15
      identical  ridge 1     9.53e-09   (cond(C) ~ 1e8: the reference's own error)
      extreme    ridge 2^40  2.39e-11
      extreme    ridge 2^54  2.28e-15
    asserted at 100 x that per group.  A wrong order, sign or transposition gives errors of order 1."""
    c = CASES[i]
    steps, _, _ = run(i)
    worst = 0.0
    for s in steps:
        d = s["direct"]
        diff = np.abs(s["b_raw"] - d)
        worst = max(worst, float(np.where(d != 0, diff / np.where(d != 0, np.abs(d), 1.0), diff).max()))
    print(T.case_id(c), "worst relative difference %.3e" % worst)
    assert worst <= BOUND[(c["kind"], c["ridge"])], worst


@pytest.mark.parametrize("i", range(len(CASES)), ids=[T.case_id(c) for c in CASES])
def test_invariants_and_branches(i):
    """M stays finite and bitwise symmetric after every step, every pay is finite; at the parity ridges b_raw is
    never negative; the case reaches the branches its parameters imply."""
    c = CASES[i]
    steps, seen, done = run(i)
    for t, s in enumerate(steps):
        assert s["finite"] and s["symmetric"] and np.isfinite(s["pay"]).all(), t
        if c is not T.CLAMP_CASE:
            assert (s["b_raw"] >= 0).all(), t
    missing = [b for b in T.case_branches(c, done) if seen[b] == 0]
    assert not missing, (missing, seen)


def test_the_clamp_case_takes_a_negative_b_raw_once():
    """N3-L5-K16-extreme-bern (seed 164) at ridge 1: |phi|^2 = 2^58 against ridge 1 cancels in the update, b_raw
    goes negative on a scored step (step 9, inside the GPU test's 12) and is paid as 0; everything stays finite
    and symmetric (the test above)."""
    steps, seen, _ = run(CASES.index(T.CLAMP_CASE))
    negative = [t for t, s in enumerate(steps) if (s["b_raw"] < 0).any()]
    assert negative == [9] and seen["clamp"] == 1, (negative, seen)
    for s in steps:
        assert (s["pay"] >= 0).all()


def test_hand_written_values():
    ridge = 4.0
    tw = T.Elliptical(2, ridge, beta=0.5)
    phi = np.zeros((2, 16), np.int32)
    phi[0, :3] = (3, -4, 12)                                  # |phi|^2 = 169
    phi[1, 5] = 2                                             # |phi|^2 = 4
    sq = np.array([169.0, 4.0])
    rew = np.array([1.0, -2.0], np.float32)
    r, bonus = tw.step(phi, np.zeros(2, np.uint8), rew)       # an episode's first step pays 0
    assert (bonus == 0).all() and (tw.eb == 0).all() and np.array_equal(r, rew)
    assert np.array_equal(tw.b_raw, sq / ridge) and tw.count.tolist() == [1, 1]
    r, bonus = tw.step(phi, np.array([0, 1], np.uint8), rew)  # the repeat pays |phi|^2 / (ridge + |phi|^2)
    want = sq / (ridge + sq)
    assert np.abs(tw.eb - want).max() <= 1e-15, tw.eb - want
    assert np.array_equal(bonus, tw.eb.astype(np.float32))
    assert np.array_equal(r, rew + (0.5 * tw.eb).astype(np.float32))
    assert tw.count.tolist() == [2, 0]                        # env 1 ended: diag(1 / ridge) exactly
    assert np.array_equal(tw.minv[1], np.eye(16) / ridge) and not np.signbit(tw.minv[1]).any()
    assert not np.array_equal(tw.minv[0], np.eye(16) / ridge)
    r, bonus = tw.step(phi, np.zeros(2, np.uint8), rew)
    assert bonus[1] == 0 and abs(tw.eb[0] - 169.0 / (ridge + 2 * 169.0)) <= 1e-15
    assert tw.seen == {"first_step": 3, "reset": 1, "clamp": 0, "fresh": 2, "in_span": 1}
    tw.count[:] = T.INT32_MAX                                 # the count saturates
    tw.step(phi, np.zeros(2, np.uint8), rew)
    assert tw.count.tolist() == [T.INT32_MAX] * 2


def test_nan_is_paid_as_zero():
    tw = T.Elliptical(1, 1.0)
    tw.count[:] = 3
    tw.minv[0, 0, 0] = np.nan
    phi = np.ones((1, 16), np.int32)
    assert tw.bonus_step(phi, np.zeros(1, np.uint8)).tolist() == [0.0] and np.isnan(tw.b_raw[0])
    assert tw.seen["clamp"] == 1


# ---------------------------------------------------------------------------------------------------- keywords
def test_kind_is_popped_first_and_the_defaults_are_unchanged():
    import buffer
    assert buffer.ELLIPTICAL_DEFAULTS == {"ridge": 2.0 ** 30, "beta": 0.1, "frames": "last"} == T.DEFAULTS
    assert buffer.EPISODIC_DEFAULTS == E.DEFAULTS and "kind" not in buffer.EPISODIC_DEFAULTS
    import ngu_twin
    assert buffer.NGU_DEFAULTS == ngu_twin.DEFAULTS and "kind" not in buffer.NGU_DEFAULTS
    kw = dict(kind="elliptical", ridge=3.0)
    assert buffer.pop_episodic_kind(kw) == "elliptical" and kw == dict(ridge=3.0)
    kw = dict(k=3)
    assert buffer.pop_episodic_kind(kw) == "knn" and kw == dict(k=3)
    for bad in ("e3b", None, 1):
        with pytest.raises(ValueError, match="kind must be one of 'knn', 'elliptical'"):
            buffer.pop_episodic_kind(dict(kind=bad, ridge=-1.0, nonsense=1))     # before any other key
    assert buffer.elliptical_config({}) == buffer.ELLIPTICAL_DEFAULTS
    assert buffer.elliptical_config({}) is not buffer.ELLIPTICAL_DEFAULTS
    assert buffer.elliptical_config(dict(ridge=7, frames="stack")) == dict(ridge=7, beta=0.1, frames="stack")
    for key in ("k", "capacity", "eps", "xi", "c", "smax", "decay", "mod_max", "kind", "rigde"):
        with pytest.raises(TypeError, match="ridge, beta, frames"):
            buffer.elliptical_config({key: 1})
    ngu = buffer.NGU_ELLIPTICAL_KEYS
    assert ngu == ("ridge", "frames", "mod_max")
    assert buffer.elliptical_config(dict(ridge=2.0, mod_max=3.0), ngu)["ridge"] == 2.0
    for key in ("beta", "k", "capacity"):
        with pytest.raises(TypeError, match="ridge, frames, mod_max"):
            buffer.elliptical_config({key: 1}, ngu)
    for ridge in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="ridge must be finite and positive"):
            buffer.elliptical_config(dict(ridge=ridge))
        with pytest.raises(ValueError, match="ridge must be finite and positive"):
            buffer.elliptical_config(dict(ridge=ridge), ngu)


def test_entry_points_refuse_bad_arguments_before_any_hip_call():
    import native
    if not os.path.exists(native.LIB_PATH):
        pytest.skip("libppox.so not built (run __graft_entry__.build())")
    lib = native.load()
    buf = np.zeros(64, np.float64)                            # host memory: never touched, nothing is launched
    p = buf.ctypes.data

    def bonus(emb=p, done=p, N=4, ridge=1.0, beta=0.1, minv=p, count=p, eb=p, rewards=p, bonus=p):
        return lib.ppox_elliptical_bonus(emb, done, N, ridge, beta, minv, count, eb, rewards, bonus, None)
    for name in ("emb", "done", "minv", "count", "eb"):
        assert bonus(**{name: None}) == -1000, name
        assert b"ppox_elliptical_bonus: null pointer" in lib.ppox_last_error()
    for kw in (dict(N=0), dict(N=-1), dict(N=2 ** 31)):
        assert bonus(**kw) == -1000 and b"N must lie" in lib.ppox_last_error(), kw
    for ridge in (0.0, -2.0, float("inf"), float("nan")):
        assert bonus(ridge=ridge) == -1000 and b"ridge" in lib.ppox_last_error(), ridge
    for beta in (float("inf"), float("-inf"), float("nan")):
        assert bonus(beta=beta) == -1000 and b"beta" in lib.ppox_last_error(), beta

    def modulate(eb=p, err=p, N=4, em=p, mod_max=5.0, ir=p, bonus=p, mod=p):
        return lib.ppox_ngu_modulate(eb, err, N, em, mod_max, ir, bonus, mod, None)
    for name in ("eb", "em", "ir", "bonus", "mod"):
        assert modulate(**{name: None}) == -1000, name
        assert b"ppox_ngu_modulate: null pointer" in lib.ppox_last_error()
    for kw in (dict(N=0), dict(N=2 ** 31), dict(mod_max=0.5), dict(mod_max=float("nan"))):
        assert modulate(**kw) == -1000, kw
        assert b"ppox_ngu_modulate" in lib.ppox_last_error() and b"null" not in lib.ppox_last_error()
    assert b"mod_max" in lib.ppox_last_error()
    assert (buf == 0).all()
