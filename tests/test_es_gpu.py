"""The ES-NSRA kernels (csrc/es.hip) over their branches, shapes and tails, against the long-double
references of tests/es_twin.py (checked on the CPU by tests/test_es_twin.py).  Every buffer a kernel
writes is a view into a sentinel-filled allocation (tests/guarded.py), pre-filled with NaN.

Where each tolerance comes from:
  evaluate      EVAL_TOL = 16 x the float64 oracle's own worst error against the long-double restatement,
                measured on the CPU over the same members (es_twin.EVAL_TOL), relative to max(1, |value|)
  noise         rtol = atol = 1e-13 against oracle.es.perturbations, the project's existing bound (test_es.py)
  env noise     exact: a float32 u01 widened to float64, minus 0.5
  update        es_twin.update_bound, the sequential-sum bound, against the long-double sum
Everything else is bitwise equality between two launches of the same kernel."""
import functools

import numpy as np
import pytest
import torch

import es_twin as ET
from guarded import Arena
from oracle import es as O

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not ET.ld_ok(), reason=ET.LD_SKIP_REASON)]

NAN = float("nan")
F64 = torch.float64
NOISE_TOL = 1e-13
CASE_PARAMS = pytest.mark.parametrize("case", ET.CASES, ids=ET.case_id)
INDEPENDENCE_CASES = [(8, 16, 12, 2), (9, 5, 7, 2), (32, 64, 64, 8)]


def _native():
    import native
    return native


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    return t.cpu().numpy()


def _eps_buffer(arena, P, n, init=NAN):
    """(P, n) float64 with three more rows of sentinel behind it: a block's idle waves (up to three past the last
    member) that lost their early return would read those, not memory the test does not own."""
    return arena.new((P, n), F64, init=init, guard=max(64, 3 * n))


def _chunk_padded(a):
    """The first len(a) rows of a device buffer padded with NaN to whole chunks of 128 members: a partial sum that
    runs past P picks up a NaN instead of reading memory the test does not own."""
    P = len(a)
    buf = torch.full(((P + 127) // 128 * 128,) + a.shape[1:], NAN, dtype=F64, device="cuda")
    buf[:P] = torch.from_numpy(np.ascontiguousarray(a))
    return buf[:P]


@functools.lru_cache(maxsize=None)
def _xi(T, D):
    xi = torch.empty(T * D, dtype=F64, device="cuda")
    _native().es_env_noise(T, D, ET.ENV_SEED, xi)
    return xi


def _evaluate(arena, case, w, eps, sigma, P, T, want_bc=True):
    """One guarded ppox_es_evaluate launch -> (fitness (P,), bc (P, 2) or None)"""
    D, H1, H2, A = case
    fit = arena.new(P, F64, init=NAN)
    bc = arena.new((P, 2), F64, init=NAN) if want_bc else None
    _native().es_evaluate(w, eps, sigma, P, D, H1, H2, A, T, ET.ENV_SEED, _xi(T, D), fit, bc)
    return fit, bc


@functools.lru_cache(maxsize=None)
def _case_run(case):
    """The P = 5 launch of a case (one full block and one block with three idle waves), eps drawn on the device,
    and its long-double reference on the downloaded eps: computed once, shared by the tests below."""
    n = ET.n_params(case)
    arena = Arena()
    w = ET.case_weights(case)
    eps = _eps_buffer(arena, ET.P_EVAL, n)
    _native().es_noise(ET.P_EVAL, n, 0, ET.GENERATION, ET.EPS_SEED, eps)
    wd = _dev(ET.flat(w))
    fit, bc = _evaluate(arena, case, wd, eps, ET.SIGMA, ET.P_EVAL, ET.T_EVAL)
    arena.check()
    mem = ET.members(w, _np(eps), ET.SIGMA)
    f_ref, b_ref = ET.evaluate_ld(mem, ET.ENV_SEED, ET.T_EVAL)
    return dict(w=w, wd=wd, eps=eps, fit=fit, bc=bc, f_ref=f_ref, b_ref=b_ref, arena=arena)


# ------------------------------------------------------------------ evaluate
@CASE_PARAMS
def test_evaluate_matches_long_double(case):
    """Fitness and behaviour of 5 members, T = 40, within EVAL_TOL of evaluate_ld; bc[:, 1] == 0 exactly at D = 1;
    nothing written outside fitness[0:5] and bc[0:10] (a missing `p >= P` return would)."""
    r = _case_run(case)
    fit, bc = _np(r["fit"]), _np(r["bc"])
    ef, eb = ET.rel_err(fit, r["f_ref"]), ET.rel_err(bc, r["b_ref"])
    print(f"es_evaluate {ET.case_id(case)}: fitness error {ef:.3e} ({ef / ET.EVAL_TOL:.3f} of EVAL_TOL), "
          f"behaviour {eb:.3e} ({eb / ET.EVAL_TOL:.3f})")
    assert np.isfinite(fit).all() and np.isfinite(bc).all()
    assert ef <= ET.EVAL_TOL and eb <= ET.EVAL_TOL, (ef, eb)
    if case[0] == 1:
        assert (bc[:, 1] == 0).all()
    else:
        assert (bc[:, 1] != 0).all()
    # the device draw is the oracle's stream (1e-13: test_es_noise_direct), so these are the members the CPU
    # measurement of EVAL_TOL ran on
    np.testing.assert_allclose(_np(r["eps"]), ET.case_members(case)[1], rtol=NOISE_TOL, atol=NOISE_TOL)
    r["arena"].check()


@pytest.mark.parametrize("case", INDEPENDENCE_CASES, ids=ET.case_id)
def test_members_are_independent(case):
    """Member p of the P = 5 launch (wave slots 0-3 of block 0, slot 0 of block 1) == a P = 1 launch on row p of
    eps, bitwise: no shared LDS slot, no wrong p * n stride."""
    r = _case_run(case)
    arena = Arena()
    for p in range(ET.P_EVAL):
        fit, bc = _evaluate(arena, case, r["wd"], r["eps"][p:p + 1], ET.SIGMA, 1, ET.T_EVAL)
        assert torch.equal(fit, r["fit"][p:p + 1]) and torch.equal(bc, r["bc"][p:p + 1]), p
    arena.check()


@pytest.mark.parametrize("case", [(1, 1, 1, 1), (8, 64, 64, 2), (11, 7, 63, 1), (32, 64, 64, 8)], ids=ET.case_id)
def test_evaluate_without_eps(case):
    """eps = None ("evaluate w itself") is within EVAL_TOL of the reference on w, and bitwise equal to eps given
    with sigma = 0 and to member 0 of a launch whose eps row is all zeros."""
    r = _case_run(case)
    arena = Arena()
    fit, bc = _evaluate(arena, case, r["wd"], None, ET.SIGMA, 1, ET.T_EVAL)
    f_ref, b_ref = ET.evaluate_ld([r["w"]], ET.ENV_SEED, ET.T_EVAL)
    ef, eb = ET.rel_err(_np(fit), f_ref), ET.rel_err(_np(bc), b_ref)
    print(f"es_evaluate eps=None {ET.case_id(case)}: {ef:.3e} {eb:.3e}")
    assert ef <= ET.EVAL_TOL and eb <= ET.EVAL_TOL, (ef, eb)
    if case[0] == 1:
        assert float(bc[0, 1]) == 0.0
    fit0, bc0 = _evaluate(arena, case, r["wd"], r["eps"], 0.0, 2, ET.T_EVAL)
    assert torch.equal(fit0, fit.expand(2)) and torch.equal(bc0, bc.expand(2, 2))
    zeros = _eps_buffer(arena, 2, ET.n_params(case), init=0.0)
    zeros[1] = r["eps"][1]
    fitz, bcz = _evaluate(arena, case, r["wd"], zeros, ET.SIGMA, 2, ET.T_EVAL)
    assert torch.equal(fitz[:1], fit) and torch.equal(bcz[:1], bc)
    assert torch.equal(fitz[1:], r["fit"][1:2]) and torch.equal(bcz[1:], r["bc"][1:2])
    arena.check()


@pytest.mark.parametrize("case", [(8, 16, 12, 2), (9, 5, 7, 2)], ids=ET.case_id)
@pytest.mark.parametrize("P", [1, 3, 4, 5, 8])
def test_population_and_episode_edges(case, P):
    """T = 1: the state starts at 0, so the weights cannot matter and the fitness is 0.02 xi[0][0] exactly as the
    oracle computes it; T = 2 within EVAL_TOL.  bc = None gives the same fitness and writes nothing else."""
    n = ET.n_params(case)
    w = ET.case_weights(case)
    eps = O.perturbations(ET.EPS_SEED, 9, np.arange(P), n)
    mem = ET.members(w, eps, ET.SIGMA)
    arena = Arena()
    wd, ed = _dev(ET.flat(w)), _eps_buffer(arena, P, n, init=eps)
    for T in (1, 2):
        fit, bc = _evaluate(arena, case, wd, ed, ET.SIGMA, P, T)
        only, none = _evaluate(arena, case, wd, ed, ET.SIGMA, P, T, want_bc=False)
        assert none is None and torch.equal(only, fit)
        if T == 1:
            f64, b64 = O.evaluate(mem, ET.ENV_SEED, 1)
            assert np.array_equal(f64, np.full(P, 0.02 * O.env_noise(ET.ENV_SEED, case[0], 0)[0]))
            assert np.array_equal(_np(fit), f64) and np.array_equal(_np(bc), b64)
        else:
            f_ref, b_ref = ET.evaluate_ld(mem, ET.ENV_SEED, T)
            assert ET.rel_err(_np(fit), f_ref) <= ET.EVAL_TOL and ET.rel_err(_np(bc), b_ref) <= ET.EVAL_TOL
            assert len(set(_np(fit).tolist())) == P  # the members differ from the second step on
    arena.check()


BAD_SIZES = {"D=0": dict(D=0), "D=33": dict(D=33), "H1=65": dict(H1=65), "H2=0": dict(H2=0), "A=9": dict(A=9),
             "T=0": dict(T=0), "P=0": dict(P=0)}


@pytest.mark.parametrize("bad", list(BAD_SIZES))
def test_evaluate_refusals(bad):
    """Sizes outside D <= 32, hidden <= 64, A <= 8, and empty P / T, raise NativeError and leave the outputs NaN."""
    native = _native()
    kw = dict(P=4, D=8, H1=16, H2=12, A=2, T=5)
    kw.update(BAD_SIZES[bad])
    arena = Arena()
    w = torch.zeros(65 * 65 * 3, dtype=F64, device="cuda")
    eps = torch.zeros(4 * 65 * 65 * 3, dtype=F64, device="cuda")
    xi = torch.zeros(40 * 33, dtype=F64, device="cuda")
    fit, bc = arena.new(4, F64, init=NAN), arena.new((4, 2), F64, init=NAN)
    with pytest.raises(native.NativeError, match="ppox_es_evaluate"):
        native.es_evaluate(w, eps, 0.1, kw["P"], kw["D"], kw["H1"], kw["H2"], kw["A"], kw["T"], 1, xi, fit, bc)
    assert torch.isnan(fit).all() and torch.isnan(bc).all()
    arena.check()


def test_evaluate_null_arguments():
    native = _native()
    arena = Arena()
    w = torch.zeros(8 * 16 + 16 * 12 + 12 * 2, dtype=F64, device="cuda")
    fit = arena.new(1, F64, init=NAN)
    for args in ((None, _xi(5, 8), fit), (w, None, fit), (w, _xi(5, 8), None)):
        with pytest.raises(native.NativeError, match="bad arguments"):
            native.es_evaluate(args[0], None, 0.1, 1, 8, 16, 12, 2, 5, ET.ENV_SEED, args[1], args[2])
    assert torch.isnan(fit).all()
    arena.check()


# ------------------------------------------------------------------ env noise
@pytest.mark.parametrize("T,D", [(1, 1), (7, 3), (33, 8), (9, 32)])
def test_env_noise_is_the_oracles_table(T, D):
    """xi[t][d] = (double)u01(word) - 0.5 is exact in float64: bitwise the oracle's table (T * D is no multiple of
    the 256-thread block; the seed has a high word)."""
    native = _native()
    arena = Arena()
    xi = arena.new(T * D, F64, init=NAN)
    native.es_env_noise(T, D, ET.ENV_SEED, xi)
    ref = np.stack([O.env_noise(ET.ENV_SEED, D, t) for t in range(T)]).reshape(-1)
    assert np.array_equal(_np(xi), ref)
    low = arena.new(T * D, F64, init=NAN)
    native.es_env_noise(T, D, ET.ENV_SEED & 0xFFFFFFFF, low)
    assert not torch.equal(low, xi)
    arena.check()
    for T_, D_ in ((0, 1), (1, 0)):
        with pytest.raises(native.NativeError):
            native.es_env_noise(T_, D_, 1, xi)


# ------------------------------------------------------------------ perturbations
def _noise(arena, P, n, member0, gen, seed):
    eps = arena.new((P, n), F64, init=NAN)
    _native().es_noise(P, n, member0, gen, seed, eps)
    return eps


@pytest.mark.parametrize("P,n", [(1, 1), (1, 2), (3, 7), (37, 301), (2, 256)])
def test_es_noise_direct(P, n):
    """Seeds (5 << 32) | 77 and 77 (the high key word k1 = seed >> 32) are each within 1e-13 of the oracle and
    differ from each other; so do two generations.  With odd n the `2q + 1 < n` store is the edge: the guard
    after the last element is intact."""
    arena = Arena()
    hi = _noise(arena, P, n, 0, 5, ET.EPS_SEED)
    lo = _noise(arena, P, n, 0, 5, 77)
    gen = _noise(arena, P, n, 0, 6, ET.EPS_SEED)
    arena.check()
    for got, seed, g in ((hi, ET.EPS_SEED, 5), (lo, 77, 5), (gen, ET.EPS_SEED, 6)):
        ref = O.perturbations(seed, g, np.arange(P), n)
        np.testing.assert_allclose(_np(got), ref, rtol=NOISE_TOL, atol=NOISE_TOL)
    assert not (hi == lo).any() and not (hi == gen).any()


@pytest.mark.parametrize("member0", [0, 20, 2 ** 31 + 3])
def test_es_noise_slices(member0):
    """Members member0 + [2, 5) drawn on their own == rows 2..4 of the draw of members member0 + [0, 8), bitwise;
    the draw is the oracle's for those global members (the counter word is the member index mod 2^32)."""
    arena = Arena()
    n = 301
    full = _noise(arena, 8, n, member0, 4, ET.EPS_SEED)
    part = _noise(arena, 3, n, member0 + 2, 4, ET.EPS_SEED)
    arena.check()
    assert torch.equal(part, full[2:5])
    ref = O.perturbations(ET.EPS_SEED, 4, member0 + np.arange(8, dtype=np.int64), n)
    np.testing.assert_allclose(_np(full), ref, rtol=NOISE_TOL, atol=NOISE_TOL)
    if member0:
        assert not (full == _noise(arena, 8, n, 0, 4, ET.EPS_SEED)).any()


def test_es_noise_grid_stride():
    """P = 5, n = 1,700,001: 4,250,005 pairs against the capped grid of 16,384 x 256 = 4,194,304 threads, so the
    last 55,701 pairs are a second pass.  The whole array is the oracle's; no NaN is left from the pre-fill."""
    P, n = 5, 1_700_001
    assert P * ((n + 1) // 2) > 16384 * 256
    arena = Arena()
    eps = _noise(arena, P, n, 0, 2, ET.EPS_SEED)
    arena.check()
    got = _np(eps)
    assert not np.isnan(got).any()
    ref = O.perturbations(ET.EPS_SEED, 2, np.arange(P), n)
    np.testing.assert_allclose(got, ref, rtol=NOISE_TOL, atol=NOISE_TOL)


def test_es_noise_refusals():
    native = _native()
    arena = Arena()
    eps = arena.new((2, 3), F64, init=NAN)
    for P, n, m0, e in ((0, 3, 0, eps), (2, 0, 0, eps), (2, 3, -1, eps), (2, 3, 0, None)):
        with pytest.raises(native.NativeError, match="ppox_es_noise"):
            native.es_noise(P, n, m0, 0, 1, e)
    assert torch.isnan(eps).all()
    arena.check()


# ------------------------------------------------------------------ update
UPDATE_CASES = [(1, 1), (2, 257), (127, 255), (128, 256), (129, 1), (257, 1000), (385, 257), (1, 1000), (385, 1),
                (129, 256), (257, 255), (128, 1000)]


def _update_inputs(P, n):
    rs = np.random.RandomState(P * 4099 + n)
    coef, eps = rs.randn(P) * 1.5, rs.randn(P, n)
    coef[3::11] = 0.0  # a few exact zeros; mixed signs otherwise
    return coef, eps


def _update(arena, coef_d, eps_d, P, n):
    native = _native()
    nbytes = native.es_update_workspace_bytes(P, n)
    assert nbytes == (P + 127) // 128 * n * 8
    ws = arena.new(nbytes // 8, F64, init=NAN)  # exactly as long as asked for
    out = arena.new(n, F64, init=NAN)
    native.es_update(eps_d, coef_d, P, n, ws, out)
    return ws, out


@pytest.mark.parametrize("P,n", UPDATE_CASES)
def test_es_update_matches_long_double(P, n):
    """delta[j] = sum_p coef[p] eps[p][j] over one chunk, exactly one, one and a member, two and a member, three
    and a member (chunks of 128), columns on both sides of the 256-thread block: every column within update_bound
    of the long-double sum, two runs bitwise equal, workspace and output guards intact."""
    coef, eps = _update_inputs(P, n)
    arena = Arena()
    cd, ed = _chunk_padded(coef), _chunk_padded(eps)
    ws, out = _update(arena, cd, ed, P, n)
    ws2, out2 = _update(arena, cd, ed, P, n)
    arena.check()
    assert torch.equal(out, out2) and torch.equal(ws, ws2) and not torch.isnan(ws).any()
    ref, bound = ET.update_ld(coef, eps), ET.update_bound(coef, eps)
    err = np.abs(_np(out).astype(np.longdouble) - ref)
    assert (bound > 0).all()
    share = float((err / bound).max())
    print(f"es_update P={P} n={n}: worst error {share:.4f} of update_bound")
    assert (err <= bound).all(), share
    # the last chunk's partial sums are its own members', not the clamped-away ones
    c0 = (P - 1) // 128 * 128
    last = ET.update_ld(coef[c0:], eps[c0:])
    assert (np.abs(_np(ws)[-n:].astype(np.longdouble) - last) <= ET.update_bound(coef[c0:], eps[c0:])).all()


def test_es_update_refusals():
    native = _native()
    P, n = 129, 257
    coef, eps = _update_inputs(P, n)
    cd, ed = _chunk_padded(coef), _chunk_padded(eps)
    arena = Arena()
    ws = arena.new(native.es_update_workspace_bytes(P, n) // 8, F64, init=NAN)
    out = arena.new(n, F64, init=NAN)
    with pytest.raises(native.NativeError, match="workspace too small"):
        native.es_update(ed, cd, P, n, ws[:-1], out)  # 8 bytes short
    for e, c, w, o in ((None, cd, ws, out), (ed, None, ws, out), (ed, cd, ws, None)):
        with pytest.raises(native.NativeError, match="bad arguments"):
            native.es_update(e, c, P, n, w, o)
    with pytest.raises(native.NativeError, match="bad arguments"):
        native.es_update(ed, cd, 0, n, ws, out)
    assert torch.isnan(out).all() and torch.isnan(ws).all()
    arena.check()


def test_es_update_population_too_large():
    """65,535 chunks is the grid's y limit: one member more is refused before anything is launched."""
    native = _native()
    P = 65535 * 128 + 1
    eps = torch.zeros(P, dtype=F64, device="cuda")
    arena = Arena()
    ws = arena.new(native.es_update_workspace_bytes(P, 1) // 8, F64, init=NAN)
    out = arena.new(1, F64, init=NAN)
    with pytest.raises(native.NativeError, match="population too large"):
        native.es_update(eps, eps, P, 1, ws, out)
    assert torch.isnan(out).all() and torch.isnan(ws).all()
    arena.check()


# ------------------------------------------------------------------ through the class
def _es(env_id, hidden, P=6, T=40, seed=(3 << 32) | 5):
    import evolution_strategies as ES
    np.random.seed(11)
    es = ES.EvolutionStrategy(env_id, hidden_sizes=list(hidden), population_size=P, sigma=0.1, learning_rate=0.01,
                              seed=seed, episode_len=T)
    es.weights = [w / np.sqrt(w.shape[0]) for w in es.weights]  # fan-in scaled: see es_twin
    return es


CLASS_ENVS = {"Hopper-v2": (11, 3), "BipedalWalker-v3": (24, 4), "InvertedPendulum-v2": (4, 1)}


@pytest.mark.parametrize("hidden", [(7, 63), (64, 64)], ids=["7x63", "64x64"])
@pytest.mark.parametrize("env_id", list(CLASS_ENVS))
def test_class_evaluates_the_env_shapes(env_id, hidden):
    """EvolutionStrategy on the env ids that run es_eval_kernel<32, 8> (and InvertedPendulum, <8, 2>):
    _get_rewards on the perturbed members, evaluate and get_behavior_char on the weights and on member 4's, within
    EVAL_TOL of evaluate_ld."""
    es = _es(env_id, hidden)
    D, A = CLASS_ENVS[env_id]
    assert es.sizes == [D, *hidden, A] and es.T == 40
    assert np.array_equal(_np(es.xi).reshape(40, D), np.stack([O.env_noise(es.env_seed, D, t) for t in range(40)]))
    es.generation = 2
    pop = es._get_population()
    assert tuple(pop.shape) == (6, es.n_params)
    rewards = es._get_rewards(None, pop)
    mem = ET.members(es.weights, _np(pop), es.SIGMA)
    f_ref, b_ref = ET.evaluate_ld(mem, es.env_seed, 40)
    f1, b1 = ET.evaluate_ld([es.weights], es.env_seed, 40)
    errs = (ET.rel_err(rewards, f_ref), ET.rel_err(es.evaluate(es.weights), f1[0]),
            ET.rel_err(es.get_behavior_char(es.weights), b1),
            ET.rel_err(es.evaluate(mem[4]), f_ref[4]), ET.rel_err(es.get_behavior_char(mem[4]), b_ref[4:5]))
    print(f"ES class {env_id} {hidden}: errors {errs[0]:.3e} {errs[1]:.3e} {errs[2]:.3e} of EVAL_TOL {ET.EVAL_TOL:.3e}")
    assert rewards.shape == (6,) and es.get_behavior_char(es.weights).shape == (1, 2)
    assert max(errs) <= ET.EVAL_TOL, errs


def test_class_plain_es_update_three_chunks():
    """_update_weights(rewards, eps, None), the plain-ES branch (coef = normalised rewards), at P = 300: three
    chunks, the last of 44 members.  Against the reference rule w + lr / (P sigma) P^T r in long double, within
    update_bound x the update factor.  (The host's own two roundings, of factor x delta and of the sum with w,
    are at most 2^-52 max|w|, which is asserted to be a small part of the bound for these inputs.)"""
    P = 300
    es = _es("Hopper-v2", (7, 63), P=P)
    eps = es._get_population()
    rewards = np.random.RandomState(1).randn(P) * 2 + 0.5
    before = ET.flat(es.weights)
    shapes = [w.shape for w in es.weights]
    es._update_weights(rewards, eps, None)
    r = (rewards - rewards.mean()) / rewards.std()
    f = 0.01 / (P * 0.1)
    e = _np(eps)
    ref = before.astype(np.longdouble) + np.longdouble(f) * ET.update_ld(r, e)
    tol = f * ET.update_bound(r, e)
    assert 2.0 ** -52 * np.abs(before).max() < 0.25 * tol.min()
    after = ET.flat(es.weights)
    err = np.abs(after.astype(np.longdouble) - ref)
    print(f"ES class plain update P=300: worst error {float((err / tol).max()):.4f} of update_bound x factor")
    assert (err <= tol).all() and [w.shape for w in es.weights] == shapes
    assert (after != before).all()
    assert es.learning_rate == 0.01 * 0.9995  # decayed once


def test_class_constant_rewards_change_nothing():
    es = _es("InvertedPendulum-v2", (7, 63))
    eps = es._get_population()
    before = [w.copy() for w in es.weights]
    es._update_weights(np.full(6, 1.25), eps, None)
    es._update_weights(np.full(6, -3.0), eps, 0.5)
    assert all(np.array_equal(a, b) for a, b in zip(es.weights, before)) and es.learning_rate == 0.01


def test_class_refuses_other_policies():
    import evolution_strategies as ES
    for hidden in ([65, 8], [8, 8, 8]):
        with pytest.raises(ValueError, match="two hidden layers"):
            ES.EvolutionStrategy("Hopper-v2", hidden_sizes=hidden, population_size=4, episode_len=5)
