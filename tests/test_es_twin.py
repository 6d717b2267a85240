"""CPU checks of the references the ES and synthetic-env GPU tests lean on (tests/es_twin.py,
tests/synth_env_twin.py): the long-double restatement of the ES episode against the float64 oracle,
where EVAL_TOL comes from and that it cannot hide an indexing error, the update bound, and the
vector-env twin against oracle.philox on the pieces they share."""
import numpy as np
import pytest

import es_twin as ET
import synth_env_twin as ST
from oracle import es as O
from oracle import philox as PH

needs_ld = pytest.mark.skipif(not ET.ld_ok(), reason=ET.LD_SKIP_REASON)


@pytest.fixture(scope="module")
def oracle_errors():
    return {case: ET.oracle_error(case) for case in ET.CASES}


@needs_ld
def test_eval_tol_is_16x_the_oracles_own_error(oracle_errors):
    """EVAL_TOL >= 16 x the float64 oracle's worst error against evaluate_ld over CASES (fitness and behaviour),
    and that worst error is at most 1e-13: the table is well conditioned."""
    worst = max(max(e) for e in oracle_errors.values())
    print("oracle vs long double, (fitness, behaviour):", {ET.case_id(c): e for c, e in oracle_errors.items()})
    assert ET.EVAL_TOL == 16 * ET.ORACLE_WORST
    assert ET.EVAL_TOL >= 16 * worst, (ET.EVAL_TOL, worst)
    assert worst <= 1e-13, worst


@needs_ld
def test_evaluate_ld_is_the_oracle_in_wider_arithmetic():
    """At T = 1 the state starts at 0 and the action is tanh(0): both programs return 0.02 xi[0][0], the float64
    one rounded once (half an ulp from the long-double one); the behaviour's second column is 0 at D = 1."""
    for case in (ET.CASES[0], ET.CASES[3]):
        _, _, mem = ET.case_members(case)
        f64, b64 = O.evaluate(mem, ET.ENV_SEED, 1)
        f, b = ET.evaluate_ld(mem, ET.ENV_SEED, 1)
        xi0 = O.env_noise(ET.ENV_SEED, case[0], 0)
        assert np.array_equal(f64, np.full(len(mem), 0.02 * xi0[0]))
        assert ET.rel_err(f64, f) <= 2.0 ** -53
        assert ET.rel_err(ET.behaviour64(b64, case[0]), b) <= 2.0 ** -53
    assert (ET.evaluate_ld(ET.case_members(ET.CASES[0])[2], ET.ENV_SEED, 5)[1][:, 1] == 0).all()


@pytest.mark.parametrize("case", ET.CASES, ids=ET.case_id)
def test_tolerance_cannot_hide_an_indexing_error(case):
    """Swapping the first and last entry of member 0's W1 (scaling W0 by 1.001 where W1 has one entry) moves
    the oracle's fitness by more than 1000 x EVAL_TOL."""
    _, _, mem = ET.case_members(case)
    f0, _ = O.evaluate(mem[:1], ET.ENV_SEED, ET.T_EVAL)
    w = [x.copy() for x in mem[0]]
    if w[1].size > 1:
        v = w[1].reshape(-1)
        v[0], v[-1] = v[-1], v[0]
    else:
        w[0] = w[0] * 1.001
    f1, _ = O.evaluate([w], ET.ENV_SEED, ET.T_EVAL)
    assert abs(f1[0] - f0[0]) > 1000 * ET.EVAL_TOL * max(1.0, abs(f0[0])), abs(f1[0] - f0[0])


@needs_ld
@pytest.mark.parametrize("P,n", [(1, 1), (2, 7), (129, 33), (385, 257), (5000, 3)])
def test_update_ld_and_bound(P, n):
    """numpy's float64 coef @ eps (a reordered sum of the same rounded products) stays inside update_bound of
    update_ld; the bound is tight enough to notice one dropped member."""
    rs = np.random.RandomState(P * 1000 + n)
    coef, eps = rs.randn(P), rs.randn(P, n)
    coef[::7] = 0.0
    ref, bound = ET.update_ld(coef, eps), ET.update_bound(coef, eps)
    err = np.abs((coef @ eps).astype(np.longdouble) - ref)
    assert (err <= bound).all(), float((err / np.maximum(bound, 1e-300)).max())
    if P > 1:
        dropped = np.abs((coef[:-1] @ eps[:-1]).astype(np.longdouble) - ref)
        assert (dropped > bound).all()
    else:
        assert coef[0] == 0.0 and (ref == 0).all() and (bound == 0).all()


def test_update_bound_gamma():
    """gamma = (P+1) u / (1 - (P+1) u) on |coef| . |eps|"""
    b = ET.update_bound(np.array([2.0, -3.0, 0.0]), np.array([[1.0, -1.0], [0.5, 2.0], [9.0, 9.0]]))
    g = 4 * 2.0 ** -53 / (1 - 4 * 2.0 ** -53)
    assert np.array_equal(b, g * np.array([3.5, 8.0]))


# ------------------------------------------------------------------ the vector-env twin
@pytest.mark.parametrize("D", [1, 3, 4, 5, 11, 24])
def test_vec_twin_shares_the_atari_streams(D):
    """The vector env's observation words are the first D uint32 words of the Atari frame at the same counter
    (block, env, step, action), and its done draw is oracle.philox.events' one."""
    seed, n, off = (0xABCD << 32) | 99, 7, 100
    ids = np.arange(off, off + n)
    env = ST.SyntheticVec(n, D, seed, p_done=0.2, max_len=0, env_offset=off)
    frame0 = PH.atari_frame(seed, ids, 0, np.full(n, PH.RESET_ACTION))
    words = np.ascontiguousarray(frame0).view("<u4")[:, :D]
    obs = env.reset()
    assert obs.dtype == np.float32 and obs.shape == (n, D)
    assert np.array_equal(obs, PH.u01(words) * np.float32(2) - np.float32(1))
    assert (obs >= -1).all() and (obs < 1).all()
    rs = np.random.RandomState(D)
    for k in range(1, 6):
        a = rs.randint(0, 3, n).astype(np.int32)
        obs, rew, done = env.step(a)
        words = np.ascontiguousarray(PH.atari_frame(seed, ids, k, a)).view("<u4")[:, :D]
        assert np.array_equal(obs, PH.u01(words) * np.float32(2) - np.float32(1)), k
        assert np.array_equal(done, PH.events(seed, ids, k, a, 0.0, 0.2)[1]), k
        assert (rew == 1).all()


def test_vec_twin_box_actions_are_zero_and_max_len_ends_episodes():
    seed, n = 5, 4
    box = ST.SyntheticVec(n, 3, seed, max_len=3, discrete=False)
    zero = ST.SyntheticVec(n, 3, seed, max_len=3)
    box.reset(), zero.reset()
    for k in range(1, 8):
        o1, _, d1 = box.step(np.full(n, 2))           # ignored
        o2, _, d2 = zero.step(np.zeros(n, np.int32))
        assert np.array_equal(o1, o2) and np.array_equal(d1, d2)
        assert d1.all() == (k % 3 == 0) and d1.any() == (k % 3 == 0)
        assert (box.done_len == (3 if k % 3 == 0 else 0)).all()
