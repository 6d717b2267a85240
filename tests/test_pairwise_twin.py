"""CPU twins of csrc/rms.hip's host-checkable claims (no GPU).

1. pairwise_sum_block's leaf enumeration, restated in Python: the leaves summed as pw_leaf
   sums them and combined in the kernel's order give np.sum bit for bit (float32 and float64)
   up to 262,144 elements.  That holds only with one pairwise tree per 8192-element ufunc
   buffer, the trees' sums added in order: numpy's reduction never hands its pairwise routine
   more than one buffer, and a single tree over 65,537 elements is 1 ulp off on most draws.
   The leaf count peaks at 2049 for n <= 262,144 (the two float32 entry points' cap), and
   ppox_vecnorm_reward admits exactly the n with at most MAX_LEAVES leaves.  Before it counted
   the leaves it admitted every n <= MAX_LEAVES * PW_BLOCK = 524,288; with the single tree it
   then built, 28,665 sizes from 491,529 upward split into more than 4096 leaves (524,287 into
   4097), and thread 0 of the kernel wrote leaf_off[4096] and beyond, past its shared arrays.
   With one tree per buffer 441 sizes from 523,785 upward still would.
2. numpy's own variance error on the uint8 batches of tests/test_rms_gpu.py: np.var lies within
   rows * 2^-53 relative of the exact rational variance about the rounded mean, so the
   rtol 1e-12 that the merged variance is held to there is the reference's error (4.6e-13 at
   4099 rows), not slack for the kernel.
Reference: numpy's add.reduce / pairwise_sum (behind np.mean / np.var in util.py:20-28)."""
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import rms_u8_cases as U8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = open(os.path.join(ROOT, "ppo-exploration_amd", "csrc", "rms.hip")).read()
NP_BUF = int(re.search(r"constexpr int NP_BUF = (\d+);", _SRC).group(1))
PW_BLOCK = int(re.search(r"constexpr int PW_BLOCK = (\d+);", _SRC).group(1))
MAX_LEAVES = int(re.search(r"constexpr int MAX_LEAVES = (\d+);", _SRC).group(1))
F32_CAP = MAX_LEAVES * 64  # ppox_rms_scale_int_rewards, ppox_rms_update_f32 with one column
OLD_VECNORM_CAP = MAX_LEAVES * PW_BLOCK
VECNORM_MAX_N = OLD_VECNORM_CAP  # 64 full chunks of 64 leaves: the largest n ppox_vecnorm_reward admits
F32_CAP_PEAK, CHUNKED_FIRST_OVER, CHUNKED_OVER = 2049, 523_785, 441  # pinned: see the tests that use them

SIZES = (1, 7, 8, 9, 128, 129, 136, 1025, 65_537, 262_144)


def tree_leaves(off, n):
    """numpy's pairwise split of one block: (offset, length) in visiting order (left first)."""
    out, st = [], [(off, n)]
    while st:
        off, k = st.pop()
        if k <= PW_BLOCK:
            out.append((off, k))
            continue
        n2 = k // 2
        n2 -= n2 % 8
        st.append((off + n2, k - n2))  # right pushed first -> left visited first
        st.append((off, n2))
    return out


def leaves(n):
    """pairwise_sum_block's enumeration: one tree per NP_BUF-element chunk, in order."""
    return [lf for c0 in range(0, n, NP_BUF) for lf in tree_leaves(c0, min(NP_BUF, n - c0))]


def pw_leaf(x, off, n):
    """pw_leaf: a plain loop below 8 elements, else 8 accumulators, their tree, then the tail."""
    T = x.dtype.type
    if n < 8:
        res = T(0)
        for i in range(n):
            res = res + x[off + i]
        return res
    r = x[off:off + 8].copy()
    i = 8
    while i < n - n % 8:
        r = r + x[off + i:off + i + 8]
        i += 8
    res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
    while i < n:
        res = res + x[off + i]
        i += 1
    return res


def pairwise_sum_block(x):
    """Leaves summed independently; per chunk the post-order combine with a value stack, the
    chunks' sums added in order to an accumulator that starts at zero."""
    n = len(x)
    sums = [pw_leaf(x, off, k) for off, k in leaves(n)]
    result, k = x.dtype.type(0), 0
    for c0 in range(0, n, NP_BUF):
        st, vs = [[c0, min(NP_BUF, n - c0), 0]], []
        while st:
            f = st[-1]
            if f[1] <= PW_BLOCK:
                vs.append(sums[k])
                k += 1
                st.pop()
                continue
            n2 = f[1] // 2
            n2 -= n2 % 8
            if f[2] == 0:
                f[2] = 1
                st.append([f[0], n2, 0])
            elif f[2] == 1:
                f[2] = 2
                st.append([f[0] + n2, f[1] - n2, 0])
            else:
                b = vs.pop()
                a = vs.pop()
                vs.append(a + b)
                st.pop()
        assert len(vs) == 1
        result = result + vs[0]
    assert k == len(sums)
    return result


def tree_counts(nmax):
    """Leaf count of one pairwise tree over n elements, for every n <= nmax, by the split's recurrence."""
    cnt = np.ones(nmax + 1, np.int64)
    cnt[0] = 0
    for n in range(PW_BLOCK + 1, nmax + 1):
        n2 = n // 2
        n2 -= n2 % 8
        cnt[n] = cnt[n2] + cnt[n - n2]
    return cnt


@pytest.fixture(scope="module")
def tree():
    return tree_counts(OLD_VECNORM_CAP + 1000)


def kernel_count(tree, n):
    """Leaves pairwise_sum_block enumerates: 64 per full chunk and the last chunk's tree."""
    return (n // NP_BUF) * int(tree[NP_BUF]) + int(tree[n % NP_BUF])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n", SIZES)
def test_leaf_twin_equals_numpy_sum(n, dtype):
    rs = np.random.RandomState(n)
    for scale in (1.0, 1e3):
        x = (rs.randn(n) * scale).astype(dtype)
        got = pairwise_sum_block(x)
        assert got.dtype == dtype
        assert got.tobytes() == np.sum(x).tobytes(), (n, dtype, scale)
        q = (x - np.mean(x)) ** 2  # the second pass of np.var
        assert pairwise_sum_block(q).tobytes() == np.sum(q).tobytes(), (n, dtype, scale)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_one_tree_is_not_numpy_above_one_buffer(dtype):
    """Why the enumeration is chunked: a single pairwise tree over more than np.getbufsize()
    elements is not what np.sum computes (1 ulp apart on most draws), up to it it is."""
    assert np.getbufsize() == NP_BUF

    def one_tree(x):
        sums = {off: pw_leaf(x, off, k) for off, k in tree_leaves(0, len(x))}

        def rec(off, k):
            if k <= PW_BLOCK:
                return sums[off]
            n2 = k // 2
            n2 -= n2 % 8
            return rec(off, n2) + rec(off + n2, k - n2)
        return rec(0, len(x))
    differ = 0
    for seed in range(8):
        x = np.abs(np.random.RandomState(seed).randn(65_537)).astype(dtype)
        assert one_tree(x[:NP_BUF]).tobytes() == np.sum(x[:NP_BUF]).tobytes()
        differ += one_tree(x).tobytes() != np.sum(x).tobytes()
        assert pairwise_sum_block(x).tobytes() == np.sum(x).tobytes()
    assert differ > 0


def test_counts_match_the_enumerated_leaves(tree):
    for n in SIZES + (8191, 8192, 8193, 8321, 262_143, 491_529, 524_287, 524_288):
        lv = leaves(n)
        assert len(lv) == kernel_count(tree, n)
        assert len(tree_leaves(0, n)) == tree[n]
        assert lv[0][0] == 0 and all(a[0] + a[1] == b[0] for a, b in zip(lv, lv[1:])) and sum(lv[-1]) == n
        # why n <= 64 * MAX_LEAVES is safe: only a last chunk of <= PW_BLOCK elements makes a leaf below 64
        small = [k for _, k in lv if k < 64]
        assert not small or (len(small) == 1 and lv[-1][1] == small[0] and n % NP_BUF <= PW_BLOCK)


def test_f32_cap_leaf_counts(tree):
    """One tree peaks at 2049 leaves for n <= 262,144, and so does the chunked enumeration (31 * 64 + 65)."""
    assert F32_CAP == 262_144
    assert tree[:F32_CAP + 1].max() == 2049 <= MAX_LEAVES
    chunked = max(kernel_count(tree, n) for n in range(1, F32_CAP + 1))
    assert chunked == F32_CAP_PEAK <= MAX_LEAVES


def test_old_vecnorm_cap_admitted_overflowing_sizes(tree):
    """Defect 2 in numbers: what n <= MAX_LEAVES * PW_BLOCK let through when the kernel built one
    tree over all n elements, and what it would let through with one tree per chunk."""
    over = np.nonzero(tree[:OLD_VECNORM_CAP + 1] > MAX_LEAVES)[0]
    assert over[0] == 491_529 and len(over) == 28_665
    assert tree[524_287] == 4097 and tree[524_288] == 4096
    assert tree[OLD_VECNORM_CAP + 1:].min() > MAX_LEAVES
    over = [n for n in range(OLD_VECNORM_CAP - NP_BUF, OLD_VECNORM_CAP + 1) if kernel_count(tree, n) > MAX_LEAVES]
    assert over[0] == CHUNKED_FIRST_OVER and len(over) == CHUNKED_OVER
    assert max(kernel_count(tree, n) for n in range(1, OLD_VECNORM_CAP - NP_BUF + 1)) <= MAX_LEAVES


def _vecnorm_admits(lib, n):
    """The size check comes before every other one, so null pointers reach no kernel: a refused
    size reports the leaves, an admitted one falls through to the pointer check."""
    rc = lib.ppox_vecnorm_reward(None, None, None, n, 0.99, None, None, 1.0, 1e-8, 10.0, 1, None)
    assert rc == -1000
    msg = lib.ppox_last_error()
    assert (b"pairwise leaves" in msg) != (b"bad arguments" in msg), msg
    return b"bad arguments" in msg


def test_vecnorm_reward_admits_no_overflowing_size(tree):
    import native
    if not os.path.exists(native.LIB_PATH):
        pytest.skip("libppox.so not built (run __graft_entry__.build())")
    lib = native.load()
    top = OLD_VECNORM_CAP
    refused = 0
    for n in range(top - 40_000 + 1, top + 1):  # the top 40,000 sizes, exhaustively
        ok = _vecnorm_admits(lib, n)
        assert ok == (kernel_count(tree, n) <= MAX_LEAVES), (n, kernel_count(tree, n))
        refused += not ok
    assert refused == CHUNKED_OVER
    assert _vecnorm_admits(lib, top) and _vecnorm_admits(lib, VECNORM_MAX_N)
    for n in (top + 1, top + 8, 2 * top, 2 ** 31 + 5, 2 ** 40):
        assert not _vecnorm_admits(lib, n)
    for n in (1, 129, 8193, 65_537, 262_144, 491_529):
        assert _vecnorm_admits(lib, n)


@pytest.mark.parametrize("rows", U8.ROWS)
def test_numpy_variance_error_on_the_u8_batches(rows):
    """np.var (sequential float64 over axis 0, about the rounded mean) vs the exact rational value."""
    for r, seed in U8.sequence(rows):
        _, x = U8.batch(r, seed)
        S, Q, _ = U8.exact_moments(x)
        mean, var = np.mean(x, axis=0), np.var(x, axis=0)
        bound = Fraction(r, 2 ** 53)
        assert bound < Fraction(1, 10 ** 12)
        for c in range(U8.COLS):
            m = Fraction(float(mean[c]))
            exact = (Q[c] - 2 * m * S[c] + r * m * m) / r  # sum (x - m)^2 / n, m the float64 mean
            err = abs(Fraction(float(var[c])) - exact)
            assert err <= bound * exact, (r, c, U8.KINDS[c % len(U8.KINDS)], float(err / exact) if exact else err)
            if len(set(x[:, c].tolist())) == 1:
                assert var[c] == 0.0
