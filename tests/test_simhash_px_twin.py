"""The pixel SimHash twin's own properties (CPU).  The GPU tests (test_simhash_px_gpu.py) pin the
kernels to the twin bit for bit; this file pins what the twin's definition promises: a symmetric,
zero-mean, variance-8 integer matrix, sums that fit int32, a hash that tells Catch states apart,
and projections that are exactly 0 (so the strict > of the key is exercised)."""
import numpy as np
import pytest

import simhash_px_twin as H

D = 4 * 84 * 84


@pytest.mark.parametrize("seed", [0, 1, 7])
def test_matrix_distribution(seed):
    A = H.matrix(D, seed).astype(np.int64)
    assert A.shape == (16, D)
    assert np.abs(A).max() <= 16                      # popcount(16 bits) - popcount(16 bits)
    assert np.abs(A).max() <= 13                      # measured 13 / 12 / 13 for these seeds
    assert 7.9 < A.var() < 8.1                        # binomial(16, 1/2) difference: variance 8
    assert abs(A.mean()) < 0.02                       # 0 +- 4 sigma / sqrt(16 D)
    # word d % 4 of counter d / 4: a prefix of a longer matrix is the shorter one
    assert np.array_equal(H.matrix(101, seed), A[:, :101].astype(np.int8))


def test_high_key_word_changes_the_matrix():
    assert not np.array_equal(H.matrix(256, 5), H.matrix(256, 2 ** 32 + 5))


def test_keys_definition_on_a_small_case():
    A = H.matrix(8, 0)
    obs = np.array([[0] * 8, [255] * 8, [1, 0, 0, 0, 0, 0, 0, 200]], np.uint8)
    k = H.keys(obs, A)
    assert k[0] == 0                                   # all projections 0: strict > leaves every bit clear
    rs = A.astype(np.int64).sum(axis=1)
    assert k[1] == sum(1 << b for b in range(16) if rs[b] > 0)   # bytes >= 128 count as unsigned
    p = A[:, 0].astype(np.int64) + 200 * A[:, 7].astype(np.int64)
    assert k[2] == sum(1 << b for b in range(16) if p[b] > 0)


def test_bonus_is_the_sequential_dictionary_update():
    table = H.new_table()
    cnt, bn = H.bonus(np.array([3, 3, 9, 3], np.int32), table)
    assert cnt.tolist() == [1, 2, 1, 3] and table[3] == 3 and table[9] == 1
    cnt, _ = H.bonus(np.array([9, 3], np.int32), table)
    assert cnt.tolist() == [2, 4]
    assert np.array_equal(bn, 0.1 / np.sqrt(np.array([1, 2, 1, 3], np.float64)))


def test_catch_run_discriminates_states_and_hits_zero_projections():
    """Random-policy Catch, 64 envs x 128 steps, seed 0: the hash separates most distinct frame
    stacks, some projections are exactly 0, and every sum is far inside int32."""
    stacks = H.catch_stacks(64, 128, seed=0).reshape(64 * 128, -1)
    first = {}
    for i, row in enumerate(stacks):                   # distinct rows (np.unique(axis=0) sorts 231 MB)
        first.setdefault(row.tobytes(), i)
    uniq = stacks[sorted(first.values())]
    A = H.matrix(D, 0)
    proj = H.projections(uniq, A)
    keys = H.keys(uniq, A)
    n_stacks, n_keys = len(uniq), len(np.unique(keys))
    print(f"distinct stacks {n_stacks}, distinct keys {n_keys}, ratio {n_keys / n_stacks:.3f}, "
          f"zero projections {int((proj == 0).sum())}, max |sum| {int(np.abs(proj).max())}")
    assert n_keys >= n_stacks / 2
    assert (proj == 0).any()
    assert np.abs(proj).max() < 2 ** 31
    assert 16 * 255 * D < 2 ** 31                      # the bound for any frame
