"""EvolutionStrategy(..., novelty="member"): the class logic of per-member novelty (NSR-ES), on the CPU.

The device entry points are stood in for by their CPU restatements (oracle/es.py for the perturbations, the
episodes and the P^T c; tests/es_novelty_twin.py for ppox_es_knn_novelty) — the pattern of tests/test_es_dist.py,
restated here.  Under test: the update rule on flat rewards (the stall of novelty="scalar" that DESIGN.md §8
documents, and its end), the empty-archive and zero-deviation branches, the device archive's bookkeeping, the
all-gather of the novelty in member order over ragged shards, and that the default path did not move
(tests/golden/es_novelty_scalar.npz: the host RNG state and the weights after 4 generations, recorded on the commit
before the keyword existed)."""
import contextlib
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import es_novelty_twin as T

STANDINS = ("lib", "es_env_noise", "es_noise", "es_evaluate", "es_update_workspace_bytes", "es_update",
            "es_knn_novelty")


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _oracle_device(native, flat_fitness=None, coefs=None):
    """Replace the ES entry points of `native` by CPU restatements on CPU tensors.  flat_fitness: every member's
    fitness is this constant (the behaviours stay the episodes'); coefs: a list that receives every coefficient
    vector handed to es_update."""
    from oracle import es as O

    def split(flat, sizes):
        out, off = [], 0
        for a, b in zip(sizes[:-1], sizes[1:]):
            out.append(flat[off:off + a * b].reshape(a, b))
            off += a * b
        return out

    def es_evaluate(w, eps, sigma, P, D, H1, H2, A, T, env_seed, xi, fit, bc=None, stream=None):
        wn, sizes = w.numpy(), [D, H1, H2, A]
        flats = [wn + sigma * eps[p].numpy() for p in range(P)] if eps is not None else [wn]
        f, b = O.evaluate([split(x, sizes) for x in flats], env_seed, T)
        if flat_fitness is None:
            fit.copy_(torch.from_numpy(f))
        else:
            fit.fill_(flat_fitness)
        if bc is not None:
            bc.copy_(torch.from_numpy(b))

    def es_update(eps, coef, P, n, ws, out, stream=None):
        if coefs is not None:
            coefs.append(coef.numpy().copy())
        out.copy_(torch.from_numpy(coef.numpy() @ eps.numpy()))

    def es_knn_novelty(bc, archive, K, novelty, stream=None):
        novelty.copy_(torch.from_numpy(T.novelty(bc.numpy(), archive.numpy(), K)))

    native.lib = lambda: None
    native.es_env_noise = lambda T, D, env_seed, xi, stream=None: xi.zero_()
    native.es_noise = lambda P, n, m0, gen, seed, eps, stream=None: eps.copy_(
        torch.from_numpy(O.perturbations(seed, gen, np.arange(m0, m0 + P), n)))
    native.es_evaluate = es_evaluate
    native.es_update_workspace_bytes = lambda P, n: 8
    native.es_update = es_update
    native.es_knn_novelty = es_knn_novelty


@contextlib.contextmanager
def _standins(**kw):
    import native
    missing = object()
    saved = {k: getattr(native, k, missing) for k in STANDINS}
    _oracle_device(native, **kw)
    try:
        yield native
    finally:
        for k, v in saved.items():
            if v is missing:
                delattr(native, k)
            else:
                setattr(native, k, v)


def _make(P=24, hidden=(8, 6), T_len=12, **kw):
    import evolution_strategies as ES
    np.random.seed(5)
    return ES.EvolutionStrategy("Swimmer-v3", hidden_sizes=list(hidden), population_size=P, sigma=0.1,
                                learning_rate=0.02, seed=9, episode_len=T_len, device="cpu", **kw)


def _flat(weights):
    return np.concatenate([w.reshape(-1) for w in weights])


def _brains(es, gens):
    """run(gens), recording the meta-population: returns the (brain index, weights before, weights after) of
    every generation through the hooks run() calls around the update"""
    log = []
    for name in ("_update_weights", "_update_weights_member"):
        inner = getattr(es, name, None)
        if inner is None:
            continue

        def hooked(rewards, population, arg=None, inner=inner):
            before = _flat(es.weights).copy()
            inner(rewards, population, arg)
            log.append((before, _flat(es.weights).copy(), float(es.learning_rate)))
        setattr(es, name, hooked)
    es.run(gens, log_interval=10 ** 9)
    return log


# ------------------------------------------------------------------ the stall and its end
def test_flat_rewards_still_update_with_member_novelty():
    """Every member's fitness is -200 (MountainCar short of the flag).  novelty="member": generation 0 has no
    archive and both deviations are 0, so nothing moves; from generation 1 the members' novelty differs and the
    evaluated brain's weights change, the learning rate decaying with each update."""
    with _standins(flat_fitness=-200.0):
        es = _make(novelty="member")
        log = _brains(es, 4)
    assert len(log) == 4
    before, after, lr = log[0]
    assert np.array_equal(before, after) and lr == 0.02 and es.archive[0].shape == (1, 2)
    rate = 0.02
    for g, (before, after, lr) in enumerate(log[1:], 1):
        assert not np.array_equal(before, after), f"generation {g}: flat rewards, a non-empty archive, no update"
        rate *= es.decay
        assert lr == rate
    assert es.member_novelty.shape == (24,) and es.member_novelty.std() > 0
    assert es._archive_n == 4 and np.array_equal(es._archive_dev[:4].numpy(), np.concatenate(es.archive))


def test_flat_rewards_stall_in_scalar_mode():
    """The same inputs with novelty="scalar" (and with the keyword left out): no generation changes a weight and
    the learning rate never decays — the stall DESIGN.md §8 documents."""
    for kw in (dict(novelty="scalar"), {}):
        with _standins(flat_fitness=-200.0):
            es = _make(**kw)
            log = _brains(es, 4)
        assert len(log) == 4 and es.novelty_mode == "scalar"
        for before, after, lr in log:
            assert np.array_equal(before, after) and lr == 0.02
        assert es.member_novelty is None and es._archive_n == 0 and len(es.archive) == 4


def test_both_deviations_zero_is_the_early_return():
    coefs = []
    with _standins(coefs=coefs):
        es = _make(novelty="member")
        pop = es._get_population()
        w0 = _flat(es.weights).copy()
        es._update_weights_member(np.full(24, -200.0), pop, np.full(24, 0.25))
        es._update_weights_member(np.full(24, -200.0), pop, None)
    assert coefs == [] and np.array_equal(_flat(es.weights), w0) and es.learning_rate == 0.02


def test_coefficients():
    """c = ((1 - nu) z(r) + nu z(n)) / 2 with numpy's population std; z(n) = 0 while the archive is empty
    (member_novelty None) or where the novelty's deviation is 0, z(r) = 0 on flat rewards."""
    rs = np.random.RandomState(3)
    r, n = rs.randn(24) * 7 - 3, np.abs(rs.randn(24)) + 0.1
    zr, zn = (r - r.mean()) / r.std(), (n - n.mean()) / n.std()
    coefs = []
    with _standins(coefs=coefs):
        es = _make(novelty="member", novelty_param=0.3)
        pop = es._get_population()
        es._update_weights_member(r, pop, None)
        es._update_weights_member(r, pop, np.full(24, 0.5))
        es._update_weights_member(r, pop, n)
        es._update_weights_member(np.full(24, -200.0), pop, n)
    rate = 0.02
    for _ in range(4):
        rate *= es.decay
    nu = 0.3
    assert len(coefs) == 4 and es.learning_rate == rate
    assert np.array_equal(coefs[0], (1 - nu) * zr / 2)
    assert np.array_equal(coefs[1], (1 - nu) * zr / 2)
    assert np.array_equal(coefs[2], ((1 - nu) * zr + nu * zn) / 2)
    assert np.array_equal(coefs[3], nu * zn / 2)


def test_archive_mirror_grows_by_doubling():
    with _standins():
        es = _make(novelty="member")
        rows = np.random.RandomState(0).randn(40, 2)
        caps = []
        for row in rows:
            es._archive_push(torch.from_numpy(row).reshape(1, 2))
            caps.append(es._archive_dev.shape[0])
    assert sorted(set(caps)) == [16, 32, 64] and es._archive_n == 40
    assert np.array_equal(es._archive_dev[:40].numpy(), rows)


def test_member_novelty_is_the_twin_on_the_members_behaviour():
    """_get_rewards_novelty: one evaluation launch that also asks for bc, then es_knn_novelty with K = self.K on
    this rank's members against the rows pushed so far; None while the archive is empty."""
    seen = []
    with _standins() as native:
        es = _make(novelty="member")
        inner = native.es_evaluate

        def counted(w, eps, sigma, P, D, H1, H2, A, T_len, env_seed, xi, fit, bc=None, stream=None):
            inner(w, eps, sigma, P, D, H1, H2, A, T_len, env_seed, xi, fit, bc)
            seen.append((P, None if bc is None else bc.numpy().copy()))
        native.es_evaluate = counted
        pop = es._get_population()
        r0, n0 = es._get_rewards_novelty(pop)
        rows = np.random.RandomState(1).randn(13, 2) * 0.1
        for row in rows:
            es._archive_push(torch.from_numpy(row).reshape(1, 2))
        r1, n1 = es._get_rewards_novelty(pop)
        plain = es._get_rewards(None, pop)
    assert [p for p, _ in seen] == [24, 24, 24] and seen[0][1] is not None and seen[2][1] is None
    assert n0 is None and np.array_equal(r0, r1) and np.array_equal(r0, plain)
    assert es.K == 10 and np.array_equal(n1, T.novelty(seen[1][1], rows, 10))


def test_novelty_keyword_is_checked():
    import evolution_strategies as ES
    with _standins():
        with pytest.raises(ValueError, match="'scalar' or 'member'"):
            ES.EvolutionStrategy("Swimmer-v3", [8, 6], population_size=4, device="cpu", novelty="x")


# ------------------------------------------------------------------ the default path did not move
def scalar_run():
    """4 generations of the default path on the stand-ins -> what tests/golden/es_novelty_scalar.npz records"""
    with _standins():
        es = _make()
        es.run(4, log_interval=10 ** 9)
    name, keys, pos, has_gauss, cached = np.random.get_state()
    assert name == "MT19937"
    return dict(weights=_flat(es.weights), rng_keys=keys, rng_pos=np.int64(pos), rng_has_gauss=np.int64(has_gauss),
                rng_cached=np.float64(cached), novelty_param=np.float64(es.novelty_param),
                learning_rate=np.float64(es.learning_rate), archive=np.concatenate(es.archive),
                rewards=np.array(es.rewards))


def test_scalar_mode_is_the_recorded_run(golden):
    g = golden("es_novelty_scalar")
    got = scalar_run()
    assert set(got) == set(g.files)
    for k in g.files:
        assert np.array_equal(got[k], g[k]), k


# ------------------------------------------------------------------ shards over gloo
PROBE_ARCHIVE = np.random.RandomState(77).randn(13, 2) * 0.05


def _run_member(P, gens):
    """(generation-0 novelty of the population against PROBE_ARCHIVE, per-generation (novelty vector,
    novelty_param), final weights, final novelty_param)"""
    es = _make(P=P, novelty="member")
    es.generation = 0
    for row in PROBE_ARCHIVE:
        es._archive_push(torch.from_numpy(row).reshape(1, 2))
    _, probe = es._get_rewards_novelty(es._get_population())
    sched = []
    inner = es._update_weights_member

    def rec(rewards, population, member_novelty):
        sched.append((None if member_novelty is None else member_novelty.copy(), float(es.novelty_param),
                      _flat(es.weights).copy()))
        return inner(rewards, population, member_novelty)
    es._update_weights_member = rec
    es.run(gens, log_interval=10 ** 9)
    return probe, sched, _flat(es.weights), float(es.novelty_param)


def _rank(rank, world, port, q, P, gens):
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (os.path.join(root, "tests"), os.path.join(root, "ppo-exploration_amd"), root):
        sys.path.insert(0, p)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as tdist
    tdist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import native
        _oracle_device(native)
        q.put((rank, _run_member(P, gens)))
    except Exception as e:  # surface the failure to the parent
        import traceback
        q.put((rank, traceback.format_exc() + repr(e)))
    finally:
        tdist.destroy_process_group()


@pytest.mark.parametrize("world,P", [(2, 23), (4, 30)])
def test_member_novelty_sharded_equals_one_process(world, P):
    """Ragged shards (23 over 2, 30 over 4).  Generation 0's population against a fixed archive: the all-gathered
    novelty vector is bitwise the one process's (inside run() generation 0 has no archive, so both sides hold None
    there).  Then run(4): the weights differ by the update's split sum (~1e-16), so later novelty vectors agree to
    1e-10 as test_es_dist.py holds later fitness; the same brain choices (the evaluated weights to 1e-12), the same
    novelty_param schedule, the final weights to 1e-12."""
    gens = 4
    with _standins():
        probe1, s1, w1, nu1 = _run_member(P, gens)
    assert probe1.shape == (P,) and s1[0][0] is None and all(s[0] is not None for s in s1[1:])
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _port()
    procs = [ctx.Process(target=_rank, args=(r, world, port, q, P, gens)) for r in range(world)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=600) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
    for r in range(world):
        got = res[r]
        if isinstance(got, str):
            raise AssertionError(f"rank {r}: {got}")
        probe, s, w, nu = got
        assert np.array_equal(probe, probe1), f"rank {r}: generation-0 novelty differs"
        assert len(s) == gens and s[0][0] is None
        assert [x[1] for x in s] == [x[1] for x in s1] and nu == nu1, f"rank {r}: novelty schedule differs"
        for (n, _, wb), (n1, _, wb1) in zip(s[1:], s1[1:]):
            np.testing.assert_allclose(n, n1, rtol=1e-10)
            np.testing.assert_allclose(wb, wb1, rtol=1e-12, atol=1e-12 * np.abs(wb1).max())  # the same brain
        np.testing.assert_allclose(w, w1, rtol=1e-12, atol=1e-12 * np.abs(w1).max())


# ------------------------------------------------------------------ the C entry point's refusals
def test_argument_validation_without_gpu():
    """Argument checks run before any HIP call, so they are testable on the CPU."""
    import ctypes

    import native
    if not os.path.exists(native.LIB_PATH):
        pytest.skip("libppox.so not built")
    lib = native.load()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    good = dict(bc=p, P=4, archive=p, M=4, D=2, K=10, novelty=p)
    bad = [dict(P=0), dict(P=-1), dict(M=0), dict(M=-3), dict(D=0), dict(D=9), dict(K=0), dict(K=17),
           dict(bc=None), dict(archive=None), dict(novelty=None)]
    for change in bad:
        a = dict(good, **change)
        rc = lib.ppox_es_knn_novelty(a["bc"], a["P"], a["archive"], a["M"], a["D"], a["K"], a["novelty"], None)
        assert rc == -1000, change
        assert b"ppox_es_knn_novelty" in lib.ppox_last_error()
