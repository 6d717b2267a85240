"""numpy restatement of ppox_es_knn_novelty, written from the header's paragraph (include/ppox.h), not from the
kernel (test helper, not a test module; checked on the CPU by tests/test_es_novelty_twin.py).

Everything is float64.  bc is P x D, archive M x D, S = min(K, M).  d(p, m) = sqrt of the squared differences
archive[m][j] - bc[p][j] added in index order j = 0 .. D-1, every product and sum rounded on its own (no fused
multiply-add).  novelty[p] = (the S smallest d(p, .), added in ascending order from the smallest) / S; a result
<= 1e-3 becomes 5e-3.  Equal distances are distinct entries."""
import numpy as np

THRESHOLD, FLOOR = 1e-3, 5e-3
EPS = 2.0 ** -52

# the case table of tests/test_es_novelty_gpu.py
POPS = (1, 5, 257)              # a lone wave, a block with idle waves, many blocks with idle waves in the tail
ARCHIVES = (1, 9, 63, 64, 65, 1000)  # below K; below, at and above one wave stride; many strides
DIMS = (1, 2, 3, 8)
NEIGHBOURS = (1, 10, 16)


def distances(bc, archive):
    """(P, M) float64, the index-order sum of squares"""
    bc, archive = np.asarray(bc, np.float64), np.asarray(archive, np.float64)
    P, D = bc.shape
    acc = np.zeros((P, archive.shape[0]))
    for j in range(D):
        diff = archive[None, :, j] - bc[:, None, j]
        acc = acc + diff * diff
    return np.sqrt(acc)


def raw_novelty(bc, archive, K):
    """the mean before the floor -> (P,)"""
    d = np.sort(distances(bc, archive), axis=1)
    S = min(int(K), d.shape[1])
    acc = np.zeros(d.shape[0])
    for i in range(S):  # ascending, from the smallest
        acc = acc + d[:, i]
    return acc / S


def novelty(bc, archive, K):
    raw = raw_novelty(bc, archive, K)
    return np.where(raw <= THRESHOLD, FLOOR, raw)


def bound(bc, archive, K):
    """|kernel - twin| <= (S + 2) 2^-52 twin, per member: a device sqrt that is not correctly rounded moves each
    distance by at most one ulp, and the S - 1 additions then act on inputs that differ by that much"""
    S = min(int(K), np.asarray(archive).shape[0])
    return (S + 2) * EPS * novelty(bc, archive, K)


def case_inputs(P, M, D, seed=None):
    """Random bc (P, D) and archive (M, D); a tenth of the archive rows duplicate other rows, and two queries
    (one when P = 1) are copies of archive rows"""
    rs = np.random.RandomState(1000 * P + 10 * M + D if seed is None else seed)
    archive = rs.randn(M, D)
    n = M // 10
    if n:
        perm = rs.permutation(M)
        archive[perm[:n]] = archive[rs.choice(perm[n:], n)]
    bc = rs.randn(P, D)
    for q in sorted({0, P - 1}):
        bc[q] = archive[rs.randint(0, M)]
    return bc, archive


def table():
    for P in POPS:
        for M in ARCHIVES:
            for D in DIMS:
                for K in NEIGHBOURS:
                    yield P, M, D, K
