"""The episodic bonus's numpy twin (tests/episodic_twin.py) against independent restatements, on the CPU: the
kNN against a brute-force selection, the tree sum against math.fsum, the ring and the reset on hand-written
cases, the int64 bound at the extreme embeddings, and that every case the GPU file drives reaches the branches
it is there for (so the seeds are picked here, where no GPU is needed)."""
import math

import numpy as np
import pytest

import episodic_twin as T


def _brute_knn(e, rows, K):
    """k smallest squared distances by repeatedly removing the minimum (Python integers)."""
    d = [sum((int(a) - int(b)) ** 2 for a, b in zip(e, r)) for r in rows]
    out = []
    while d and len(out) < K:
        i = min(range(len(d)), key=d.__getitem__)
        out.append(d.pop(i))
    return out


@pytest.mark.parametrize("m,K", [(0, 3), (1, 1), (1, 10), (7, 3), (40, 16), (100, 10)])
def test_knn_equals_brute_force(m, K):
    rs = np.random.RandomState(m * 31 + K)
    for trial in range(4):
        lo, hi = (-2, 3) if trial % 2 else (-T.EXTREME, T.EXTREME + 1)
        rows = rs.randint(lo, hi, (m, 16)).astype(np.int32)
        e = rs.randint(lo, hi, 16).astype(np.int32)
        dk, mean = T.knn(e, rows, K)
        exp = _brute_knn(e, rows, K)
        assert len(dk) == min(K, m) and [float(x) for x in exp] == list(dk)   # float(int): round to nearest
        s = 0.0
        for x in exp:
            s = s + float(x)
        assert mean == (s / len(exp) if exp else 0.0)
        assert all(dk[i] <= dk[i + 1] for i in range(len(dk) - 1))


@pytest.mark.parametrize("n", [0, 1, 2, 3, 64, 65, 257, 4096])
def test_tree_sum_within_the_f64_bound_of_fsum(n):
    """Pairwise summation over a tree of depth ceil(log2 n): |error| <= depth * u * sum |x| to first order
    (u = 2^-53); and the tree is the stated one (against an explicit recursion)."""
    rs = np.random.RandomState(n)
    x = rs.rand(n) * 10.0 ** rs.randint(-3, 12, n)
    got = T.tree_sum(x)
    depth = max(1, math.ceil(math.log2(max(n, 2))))
    assert abs(got - math.fsum(x)) <= 1.01 * depth * 2.0 ** -53 * math.fsum(np.abs(x))

    def rec(a):
        return float(a[0]) if len(a) == 1 else rec(a[:len(a) // 2]) + rec(a[len(a) // 2:])
    p = 1
    while p < n:
        p *= 2
    assert got == (rec(np.concatenate([x, np.zeros(p - n)])) if n else 0.0)


def test_ring_wraps_and_resets_on_done():
    st = T.Episodic(N=2, L=3, K=2)
    e = lambda a, b: np.array([[a] + [0] * 15, [b] + [0] * 15], np.int32)  # noqa: E731
    no = np.zeros(2, np.uint8)
    dk, kf, mk = st.knn_step(e(1, 10), no)
    assert kf.tolist() == [0, 0] and mk.tolist() == [0, 0] and st.count.tolist() == [1, 1]
    dk, kf, mk = st.knn_step(e(3, 10), no)
    assert kf.tolist() == [1, 1] and dk[:, 0].tolist() == [4, 0] and mk.tolist() == [4, 0]
    dk, kf, mk = st.knn_step(e(6, 20), no)
    assert kf.tolist() == [2, 2] and dk.tolist() == [[9, 25], [100, 100]] and mk.tolist() == [17, 100]
    # the ring is full: the 4th embedding takes slot 0 (the oldest), after the search that still saw it
    dk, kf, mk = st.knn_step(e(0, 0), np.array([0, 1], np.uint8))
    assert dk.tolist() == [[1, 9], [100, 100]] and st.mem[:, 0, 0].tolist() == [0, 0]
    assert st.count.tolist() == [4, 0] and st.seen["wrap"] == 2 and st.seen["reset"] == 1
    # env 0 no longer sees the overwritten 1; env 1 starts over with an empty memory, its slot 0 next
    dk, kf, mk = st.knn_step(e(1, 7), no)
    assert kf.tolist() == [2, 0] and dk[0].tolist() == [1, 4] and st.mem[0, 1, 0] == 1 and st.mem[1, 0, 0] == 7
    assert st.count.tolist() == [5, 1]


def test_capacity_one_and_k_above_capacity():
    st = T.Episodic(N=1, L=1, K=16)
    for t, v in enumerate([5, 7, 7]):
        dk, kf, mk = st.knn_step(np.full((1, 16), v, np.int32), np.zeros(1, np.uint8))
        assert kf[0] == min(t, 1) and (dk[0, 1:] == 0).all()
    assert dk[0, 0] == 0 and st.seen["k_lt_K"] == 2


def test_extreme_embeddings_do_not_overflow_int64():
    """+-(2^27 - 1): each difference below 2^28, a squared distance 16 * (2^28 - 2)^2 < 2^60, exact in int64."""
    a = np.full(16, T.EXTREME, np.int32)
    d = T.sq_dists(a, -a[None, :])
    exact = 16 * (2 * T.EXTREME) ** 2
    assert d.dtype == np.int64 and int(d[0]) == exact and exact < 2 ** 60
    dk, mean = T.knn(a, np.stack([-a, a]), 2)
    assert dk.tolist() == [0.0, float(exact)] and mean == float(exact) / 2
    with pytest.raises(AssertionError):
        T.sq_dists(np.full(16, 2 ** 27, np.int64), np.full((1, 16), -2 ** 27, np.int64))


def test_reward_formula_on_hand_values():
    st = T.Episodic(N=3, L=4, K=2, smax=1.2)
    dk = np.array([[0.0, 4.0], [2.0, 0.0], [0.0, 0.0]])
    kf = np.array([2, 1, 0], np.int32)
    rew, bonus = st.reward_step(dk, kf, np.array([2.0, 2.0, 99.0]), np.array([1.0, -1.0, 0.5], np.float32))
    assert st.dm.tolist() == [2.0, 1.0]                       # (2 + 2) / 2 valid envs; env 2 is masked out
    s0 = math.sqrt(1e-3 / (0.0 + 1e-3) + 1e-3 / ((2.0 - 8e-3) + 1e-3)) + 1e-3
    s1 = math.sqrt(1e-3 / ((1.0 - 8e-3) + 1e-3)) + 1e-3
    assert s0 <= 1.2 and bonus.tolist() == [np.float32(1 / s0), np.float32(1 / s1), 0.0]
    assert rew.tolist() == [np.float32(1.0) + np.float32(0.1 * (1 / s0)), np.float32(-1.0) + np.float32(0.1 * (1 / s1)),
                            0.5]
    rew, bonus = st.reward_step(np.zeros((3, 2)), np.array([2, 2, 2], np.int32), np.zeros(3), np.zeros(3, np.float32))
    assert st.dm.tolist() == [0.99 * 2.0 + (1.0 - 0.99) * 0.0, 2.0]
    assert bonus.tolist() == [0.0] * 3 and st.seen["s_gt_smax"] == 3   # sqrt(2) + c > 1.2


def test_replay_embeds_the_newest_frame_or_the_stack():
    rs = np.random.RandomState(0)
    obs = rs.randint(0, 256, (2, 3, 4, 2, 2)).astype(np.uint8)         # (T, N, C, H, W)
    A_last, A_stack = T.H.matrix(4, 1), T.H.matrix(16, 1)
    e = T.embed_frames(obs[0], A_last, "last")
    assert np.array_equal(e, obs[0][:, 3].reshape(3, 4).astype(np.int64) @ A_last.astype(np.int64).T)
    e = T.embed_frames(obs[0], A_stack, "stack")
    assert np.array_equal(e, obs[0].reshape(3, 16).astype(np.int64) @ A_stack.astype(np.int64).T)
    masks = np.array([[0, 1, 0], [0, 0, 0]], np.uint8)
    st = T.Episodic(3, 4, K=2)
    rew, bonus = T.replay(st, A_last, "last", obs, masks, np.zeros((2, 3), np.float32))
    assert st.count.tolist() == [2, 1, 2] and (bonus[0] == 0).all() and bonus[1, 1] == 0 and (bonus[1, [0, 2]] > 0).all()


@pytest.mark.parametrize("case", T.CASES, ids=T.case_id)
def test_cases_reach_their_branches(case):
    emb, done, rew = T.case_inputs(case)
    st = T.Episodic(case["N"], case["L"], case["K"], smax=case["smax"])
    for t in range(len(emb)):
        st.step(emb[t], done[t], rew[t])
    missing = [b for b in T.case_branches(case) if st.seen[b] == 0]
    assert not missing, (missing, st.seen)


def test_cases_cover_the_grid():
    assert {c["N"] for c in T.CASES} == {1, 3, 64, 65, 257}
    assert {(c["L"], c["K"]) for c in T.CASES} >= {(L, K) for L in (1, 2, 5, 40) for K in (1, 3, 10, 16)}
    assert {c["done"] for c in T.CASES} == {"never", "always", "bern"}
    assert {c["kind"] for c in T.CASES} == {"small", "extreme", "identical"}
    for b in ("wrap", "reset", "k_lt_K", "s_gt_smax", "dm_zero"):
        assert any(b in T.case_branches(c) for c in T.CASES), b
