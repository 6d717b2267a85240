"""ppox_es_knn_novelty (csrc/es_novelty.hip) and EvolutionStrategy(..., novelty="member") on the device, against
tests/es_novelty_twin.py (checked on the CPU by tests/test_es_novelty_twin.py).  Every buffer of a kernel launch is
a view into a sentinel-filled allocation (tests/guarded.py); the output is pre-filled with NaN.

The bound is derived, not measured: |kernel - twin| <= (S + 2) 2^-52 twin per member.  The differences, squares
and sums are the twin's operations one for one (the unit is built with fp contraction off); a device sqrt that is
not correctly rounded moves each distance by at most one ulp, the S - 1 additions then act on inputs that differ by
that much, and the division rounds once.  No member is left out: the table's novelties keep 1e-9 clear of the
floor's threshold (asserted on the CPU).  The measured worst case is printed per (P, D); on the MI355X it is 0
over the whole table and in the class tests (profiles/es_novelty/tests.log) — the derived bound stays."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import es_novelty_twin as T
from guarded import Arena

pytestmark = pytest.mark.gpu

NAN = float("nan")
F64 = torch.float64


def _native():
    import native
    return native


def _launch(bc, archive, K):
    """one guarded launch -> the (P,) device novelty"""
    arena = Arena()
    b = arena.new(bc.shape, F64, init=bc)
    a = arena.new(archive.shape, F64, init=archive)
    out = arena.new(bc.shape[0], F64, init=NAN)
    _native().es_knn_novelty(b, a, K, out)
    arena.check()
    return out


def _excess(got, bc, archive, K):
    """max over members of |kernel - twin| / bound, and of |kernel - twin| / twin"""
    want = T.novelty(bc, archive, K)
    assert np.isfinite(got).all()
    err = np.abs(got - want)
    return float((err / T.bound(bc, archive, K)).max()), float((err / want).max())


@pytest.mark.parametrize("D", T.DIMS)
@pytest.mark.parametrize("P", T.POPS)
def test_table(P, D):
    """P {1, 5, 257} x M {1, 9, 63, 64, 65, 1000} x D {1, 2, 3, 8} x K {1, 10, 16}; a tenth of the archive rows are
    copies of other rows and two queries are copies of archive rows"""
    worst, floored = 0.0, 0
    for M in T.ARCHIVES:
        bc, archive = T.case_inputs(P, M, D)
        for K in T.NEIGHBOURS:
            got = _launch(bc, archive, K).cpu().numpy()
            ratio, rel = _excess(got, bc, archive, K)
            worst = max(worst, rel)
            floored += int((got == T.FLOOR).sum())
            assert ratio <= 1.0, (P, M, D, K, ratio, rel)
    print(f"knn novelty P={P} D={D}: worst |kernel - twin| / twin {worst:.3e} over 18 cases, {floored} floored")
    assert floored >= 2  # K = 1 (and M = 1) on the copied queries


def test_shards_and_reruns():
    """P = 257 split at 100: the launch over members [m0, m1) equals those rows of the full launch bitwise, and
    two launches of the same arguments are bitwise equal"""
    for D, K in ((2, 10), (3, 16)):
        bc, archive = T.case_inputs(257, 1000, D)
        full = _launch(bc, archive, K)
        again = _launch(bc, archive, K)
        assert torch.equal(full, again)
        for m0, m1 in ((0, 100), (100, 257)):
            assert torch.equal(_launch(bc[m0:m1], archive, K), full[m0:m1]), (D, K, m0)


BAD = {"P=0": dict(P=0), "M=0": dict(M=0), "D=0": dict(D=0), "D=9": dict(D=9), "K=0": dict(K=0), "K=17": dict(K=17),
       "bc=None": dict(bc=None), "archive=None": dict(archive=None), "novelty=None": dict(novelty=None)}


@pytest.mark.parametrize("bad", list(BAD))
def test_refusals(bad):
    """refused before anything is launched: the output keeps its pre-fill"""
    native = _native()
    arena = Arena()
    b, a = arena.new((4, 9), F64, init=0.0), arena.new((4, 9), F64, init=1.0)
    out = arena.new(4, F64, init=NAN)
    kw = dict(bc=b, P=4, archive=a, M=4, D=2, K=10, novelty=out)
    kw.update(BAD[bad])
    ptr = lambda t: None if t is None else native._vp(t.data_ptr())
    with pytest.raises(native.NativeError, match="ppox_es_knn_novelty"):
        native.call("ppox_es_knn_novelty", ptr(kw["bc"]), kw["P"], ptr(kw["archive"]), kw["M"], kw["D"], kw["K"],
                    ptr(kw["novelty"]), native.stream_ptr())
    assert torch.isnan(out).all()
    arena.check()


# ------------------------------------------------------------------ through the class
def _recorded_run(env_id, novelty, gens, P, T_len, dynamics, hidden=(8, 8)):
    """run(gens) -> (per generation: rewards, evaluated weights before / after the update), the (bc, archive, K,
    kernel output) of every ppox_es_knn_novelty launch, the instance"""
    import evolution_strategies as ES
    native = _native()
    np.random.seed(11)
    es = ES.EvolutionStrategy(env_id, list(hidden), population_size=P, seed=(3 << 32) | 5, dynamics=dynamics,
                              episode_len=T_len, novelty=novelty, learning_rate=0.2)
    gen, launches = [], []
    name = "_update_weights_member" if novelty == "member" else "_update_weights"
    inner_update, inner_knn = getattr(es, name), native.es_knn_novelty

    def update(rewards, population, arg=None):
        before = np.concatenate([w.reshape(-1) for w in es.weights])
        inner_update(rewards, population, arg)
        gen.append((rewards.copy(), before, np.concatenate([w.reshape(-1) for w in es.weights])))

    def knn(bc, archive, K, out, stream=None):
        inner_knn(bc, archive, K, out, stream)
        launches.append((bc.cpu().numpy(), archive.cpu().numpy(), K, out.cpu().numpy()))
    setattr(es, name, update)
    native.es_knn_novelty = knn
    try:
        es.run(gens, log_interval=10 ** 9)
    finally:
        native.es_knn_novelty = inner_knn
    return gen, launches, es


def test_class_mountaincar_member_novelty_moves_flat_rewards():
    """MountainCar-v0, dynamics="real", P = 64, hidden (8, 8), T = 40, 3 generations: every fitness is -T, the
    per-generation novelty is the twin's on the device's own bc and archive within the bound, and the evaluated
    brain's weights change in every generation that has an archive; novelty="scalar" on the same inputs leaves
    them unchanged in every generation."""
    gen, launches, es = _recorded_run("MountainCar-v0", "member", 3, 64, 40, "real")
    assert len(gen) == 3 and len(launches) == 2 and es._archive_n == 3
    for g, (rewards, before, after) in enumerate(gen):
        assert (rewards == -40.0).all()
        assert np.array_equal(before, after) == (g == 0), g  # generation 0: no archive, both deviations 0
    for g, (bc, archive, K, got) in enumerate(launches, 1):
        assert bc.shape == (64, 2) and archive.shape == (g, 2) and K == 10
        assert np.array_equal(archive, np.concatenate(es.archive[:g]))
        ratio, rel = _excess(got, bc, archive, K)
        print(f"MountainCar member novelty, generation {g}: |kernel - twin| / twin {rel:.3e}, std {got.std():.3e}")
        assert ratio <= 1.0 and got.std() > 0
    assert np.array_equal(es.member_novelty, launches[-1][3])
    gen, launches, es = _recorded_run("MountainCar-v0", "scalar", 3, 64, 40, "real")
    assert len(gen) == 3 and launches == [] and es.learning_rate == 0.2
    for rewards, before, after in gen:
        assert (rewards == -40.0).all() and np.array_equal(before, after)


def test_class_synthetic_member_novelty():
    """Swimmer shape, dynamics="synthetic", P = 24, T = 12, 2 generations: the run completes, and generation 1's
    novelty is the twin's within the bound"""
    gen, launches, es = _recorded_run("Swimmer-v3", "member", 2, 24, 12, "synthetic", hidden=(8, 6))
    assert len(gen) == 2 and len(launches) == 1 and len(es.archive) == 2
    bc, archive, K, got = launches[0]
    assert bc.shape == (24, 2) and archive.shape == (1, 2)
    ratio, rel = _excess(got, bc, archive, K)
    print(f"Swimmer member novelty: |kernel - twin| / twin {rel:.3e}")
    assert ratio <= 1.0
    assert not np.array_equal(gen[1][1], gen[1][2])


# ------------------------------------------------------------------ two ranks on one device
PROBE_ARCHIVE = np.random.RandomState(77).randn(13, 2) * np.array([0.3, 0.02]) + np.array([-0.5, 0.0])


def _run_member(P, gens):
    """(generation-0 novelty of the population against PROBE_ARCHIVE, final weights)"""
    import evolution_strategies as ES
    np.random.seed(11)
    es = ES.EvolutionStrategy("MountainCar-v0", [8, 8], population_size=P, seed=(3 << 32) | 5, dynamics="real",
                              episode_len=40, novelty="member", learning_rate=0.2)
    es.generation = 0
    for row in PROBE_ARCHIVE:
        es._archive_push(torch.from_numpy(row).to(es.device).reshape(1, 2))
    _, probe = es._get_rewards_novelty(es._get_population())
    es.run(gens, log_interval=10 ** 9)
    return probe, np.concatenate([w.reshape(-1) for w in es.weights]), float(es.novelty_param)


def _rank(rank, world, port, q, P, gens):
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (os.path.join(root, "ppo-exploration_amd"), root):
        sys.path.insert(0, p)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as tdist
    torch.cuda.set_device(0)
    tdist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        q.put((rank, _run_member(P, gens)))
    except Exception as e:  # surface the failure to the parent
        import traceback
        q.put((rank, traceback.format_exc() + repr(e)))
    finally:
        tdist.destroy_process_group()


def test_member_novelty_two_ranks_equal_one_process():
    """Two ranks over gloo, both on cuda:0, P = 257 (shards of 128 and 129), MountainCar, T = 40, 3 generations,
    against one process: generation 0's population against a fixed archive gives the same novelty vector bitwise
    (inside run() generation 0 has no archive), the final weights agree to 1e-12."""
    P, gens, world = 257, 3, 2
    probe1, w1, nu1 = _run_member(P, gens)
    assert probe1.shape == (P,) and probe1.std() > 0
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = socket.socket()
    port.bind(("127.0.0.1", 0))
    number = port.getsockname()[1]
    port.close()
    procs = [ctx.Process(target=_rank, args=(r, world, number, q, P, gens)) for r in range(world)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=600) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
    for r in range(world):
        got = res[r]
        if isinstance(got, str):
            raise AssertionError(f"rank {r}: {got}")
        probe, w, nu = got
        assert np.array_equal(probe, probe1), f"rank {r}: generation-0 novelty differs"
        assert nu == nu1
        assert not np.array_equal(w, w1 * 0) and np.isfinite(w).all()
        np.testing.assert_allclose(w, w1, rtol=1e-12, atol=1e-12 * np.abs(w1).max())
