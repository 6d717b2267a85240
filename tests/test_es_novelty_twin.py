"""tests/es_novelty_twin.py (the restatement of ppox_es_knn_novelty that tests/test_es_novelty_gpu.py compares the
kernel with) checked on the CPU: against the class's own get_kNN at D = 2, on hand cases, and that the GPU test's
case table keeps clear of the floor's threshold and is sensitive at the scale of its bound."""
import functools

import numpy as np
import pytest

import es_novelty_twin as T


def _get_knn():
    import evolution_strategies as ES
    return ES.EvolutionStrategy.get_kNN


def test_twin_is_get_knn_bit_for_bit():
    """D = 2, random inputs: twin == get_kNN(archive, bc, S) / S with get_novelty's floor, for every member, bit
    for bit while S <= 7.  From S = 8 on get_kNN's ndarray.sum() no longer adds in ascending order (numpy sums
    eight interleaved lanes and then combines them), while the header asks for the ascending sum, so there the two
    agree to S 2^-52 relative: each is a sum of S non-negative terms, off by at most (S - 1) 2^-53 of the exact
    sum, and each division rounds once.  Measured at S = 10: 78 % of members bitwise, the rest one ulp apart."""
    get_knn = _get_knn()
    rs = np.random.RandomState(0)
    for M, K in ((1, 10), (7, 10), (10, 10), (200, 10), (200, 1), (200, 7), (200, 8), (200, 16), (1000, 10)):
        archive, bc = rs.randn(M, 2), rs.randn(40, 2)
        bc[3] = archive[M // 2]
        S = min(K, M)
        rows = [archive[m:m + 1] for m in range(M)]  # the class's list of (1, 2) behaviours
        want = np.array([get_knn(None, rows, b, S) / S for b in bc])
        want = np.where(want <= 1e-3, 5e-3, want)
        got = T.novelty(bc, archive, K)
        if S <= 7:
            assert np.array_equal(got, want), (M, K)
        else:
            assert (np.abs(got - want) <= S * T.EPS * want).all(), (M, K)
        assert (got[3] == 5e-3) == (S == 1)  # the query copied from a row takes the floor when it stands alone


def test_hand_cases():
    a = np.array([[0.0, 0.0], [3.0, 4.0], [6.0, 8.0]])
    q = np.array([[0.0, 0.0], [3.0, 4.0], [-3.0, -4.0]])
    # M = 1: the one distance, whatever K; a query on the row itself takes the floor
    assert np.array_equal(T.novelty(q, a[:1], 10), [5e-3, 5.0, 5.0])
    # M < K: S = M = 3
    assert np.array_equal(T.novelty(q, a, 10), [(0 + 5 + 10) / 3, (0 + 5 + 5) / 3, (5 + 10 + 15) / 3])
    assert np.array_equal(T.novelty(q, a, 2), [2.5, 2.5, 7.5])
    assert np.array_equal(T.novelty(q, a, 1), [5e-3, 5e-3, 5.0])
    # duplicated rows each count
    dup = np.array([[3.0, 4.0], [3.0, 4.0], [3.0, 4.0], [6.0, 8.0]])
    assert np.array_equal(T.novelty(q[:1], dup, 3), [5.0])
    assert np.array_equal(T.novelty(q[:1], dup, 4), [6.25])
    assert np.array_equal(T.novelty(q[1:2], dup, 3), [5e-3])
    # the floor's threshold is inclusive, and the floor is above it
    assert np.array_equal(T.novelty(np.array([[1e-3]]), np.array([[0.0]]), 1), [5e-3])
    assert np.array_equal(T.novelty(np.array([[1.5e-3]]), np.array([[0.0]]), 1), [1.5e-3])
    # D = 3, index-order sum: with x^2 = 0.5625 ulp(1), (1 + x^2) + x^2 = 1 + 2 ulp but (x^2 + x^2) + 1 = 1 + 1 ulp
    x, ulp = 1.5 * 2.0 ** -27, 2.0 ** -52
    zero = np.zeros((1, 3))
    assert T.novelty(zero, np.array([[1.0, x, x]]), 1)[0] == np.sqrt(1.0 + 2 * ulp)
    assert T.novelty(zero, np.array([[x, x, 1.0]]), 1)[0] == np.sqrt(1.0 + ulp)


@functools.lru_cache(maxsize=None)
def _case(P, M, D):
    return T.case_inputs(P, M, D)


def test_table_keeps_clear_of_the_threshold():
    """No novelty of the GPU test's table lies within 1e-9 of 1e-3 (before the floor), so the kernel and the twin
    take the same side for every member and the GPU test leaves none out; the copied queries do reach the floor."""
    floored = 0
    for P, M, D, K in T.table():
        bc, archive = _case(P, M, D)
        raw = T.raw_novelty(bc, archive, K)
        assert np.isfinite(raw).all() and (np.abs(raw - T.THRESHOLD) > 1e-9).all(), (P, M, D, K)
        floored += int((raw <= T.THRESHOLD).sum())
        dup = len(archive) - len(np.unique(archive, axis=0))
        assert dup == M // 10, (P, M, D, dup)  # a tenth of the rows are copies of other rows
    assert floored >= 3 * 4 * 2  # K = 1 on a copied query, in every (P, D), at least


def test_table_is_sensitive_at_the_scale_of_the_bound():
    """Moving a member's nearest archive row (with its copies) by 1e-3 in one coordinate, away from the member,
    moves that member's novelty by more than 1,000 x the bound, in every shape of the table"""
    for P, M, D, K in T.table():
        bc, archive = _case(P, M, D)
        p = P // 2  # not one of the copied queries (when P > 1)
        if P == 1:
            bc = bc + 0.25  # the lone query is a copy: take it off its row, so the distance has a slope
        base = T.raw_novelty(bc[p:p + 1], archive, K)[0]
        nearest = int(np.argmin(T.distances(bc[p:p + 1], archive)[0]))
        moved = archive.copy()
        copies = (archive == archive[nearest]).all(axis=1)
        moved[copies, 0] += 1e-3 * (1.0 if archive[nearest, 0] >= bc[p, 0] else -1.0)  # away from the query
        shifted = T.raw_novelty(bc[p:p + 1], moved, K)[0]
        S = min(K, M)
        assert abs(shifted - base) > 1000 * (S + 2) * T.EPS * base, (P, M, D, K, base, shifted)


@pytest.mark.parametrize("K", [1, 10, 16])
def test_ascending_sum(K):
    """the sum starts from the smallest distance: equal to the explicit loop over sorted distances"""
    bc, archive = _case(5, 65, 3)
    d = np.sort(T.distances(bc, archive), axis=1)
    want = []
    for row in d:
        s = 0.0
        for x in row[:K]:
            s = s + x
        want.append(s / K)
    assert np.array_equal(T.raw_novelty(bc, archive, K), want)
