"""Running moments, normalisation and VecNormalize rewards (csrc/rms.hip) at their branches, tails and limits.

Every output is carved out of a sentinel-filled buffer (tests/guarded.py) and the guards are checked.
References: numpy (np.mean / np.var and their pairwise reduction, util.py:20-44 through oracle/rms.py;
ppo.py:117, 396-398), exact rational arithmetic for the uint8 batch variance, and oracle/vecnorm.py's
arithmetic for the reward path.  tests/test_pairwise_twin.py bounds numpy's own error on the uint8 inputs."""
from fractions import Fraction

import numpy as np
import pytest
import torch

import rms_u8_cases as U8
from guarded import Arena
from oracle import rms as RM
from oracle.vecnorm import VecNormalizeNumpy

pytestmark = pytest.mark.gpu

F64 = torch.float64


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _bit_equal(got, exp, what=""):
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.dtype == exp.dtype and got.shape == exp.shape, (what, got.dtype, exp.dtype, got.shape, exp.shape)
    bad = np.nonzero(_bits(got).ravel() != _bits(exp).ravel())[0]
    assert bad.size == 0, (what, bad.size, bad[:5], got.ravel()[bad[:5]], exp.ravel()[bad[:5]])


# ----------------------------------------------------------------- uint8 columns
@pytest.mark.parametrize("rows", U8.ROWS)
def test_rms_u8_frame_like_columns(rows):
    """Constant, one-differing-row, alternating, three-outlier and uniform columns over three updates of mixed
    row counts, read through a column slice of a wider array (row_stride > cols).  batch_mean is np.mean bit for
    bit; batch_var lies within 4 * 2^-52 relative of the exact rational variance (n Q - S^2) / n^2 (one rounding
    each for the numerator's conversion above 2^53, the division and the scale) and is exactly 0 on constant
    columns; the merged mean is oracle.rms's bit for bit and the merged variance within rtol 1e-12 (numpy's own
    error, tests/test_pairwise_twin.py).
    The kernel that expanded the square in float64, Q - 2 m S + n m^2, misses the variance bound in all seven
    cases (each holds a row count that is no power of two), on the 255 ... 254, alternating and three-outlier
    columns: by up to 2.0e-9, 2.0e-11 and 3.0e-14 relative on these inputs (its formula restated in numpy
    float64); with the exact integer numerator the largest error is 1.1e-16."""
    import native
    ar = Arena()
    mean = ar.new(U8.COLS, F64, init=0.0)
    var = ar.new(U8.COLS, F64, init=1.0)
    rm = RM.RunningMoments(shape=(U8.COLS,))
    count = 1e-4
    worst = Fraction(0)
    for r, seed in U8.sequence(rows):
        wide, x = U8.batch(r, seed)
        xd = torch.from_numpy(wide).cuda()[:, U8.LEFT:U8.LEFT + U8.COLS]
        assert xd.stride(0) == U8.WIDE > U8.COLS
        ws = ar.new(native.rms_u8_workspace_bytes(r, U8.COLS), torch.uint8)
        bmean, bvar = ar.new(U8.COLS, F64), ar.new(U8.COLS, F64)
        native.rms_update_u8(xd, r, U8.COLS, U8.WIDE, mean, var, count, ws, bmean, bvar)
        count += r
        rm.update(x)
        ar.check()
        _bit_equal(bmean.cpu().numpy(), np.mean(x, axis=0), "batch_mean")
        _, _, exact = U8.exact_moments(x)
        got = bvar.cpu().numpy()
        fails = []
        for c in range(U8.COLS):
            if exact[c] == 0:
                assert got[c] == 0.0 and not np.signbit(got[c]), (r, c, got[c])
                continue
            rel = abs(Fraction(float(got[c])) - exact[c]) / exact[c]
            worst = max(worst, rel)
            if rel > Fraction(4, 2 ** 52):
                fails.append((c, U8.KINDS[c % len(U8.KINDS)], float(rel)))
        print(f"u8 rows={r}: largest relative batch_var error so far {float(worst):.3e}")
        assert not fails, (r, len(fails), fails[:8])
        _bit_equal(mean.cpu().numpy(), rm.mean, "merged mean")
        np.testing.assert_allclose(var.cpu().numpy(), rm.var, rtol=1e-12, atol=0)
        assert torch.equal(xd.cpu(), torch.from_numpy(np.ascontiguousarray(x)))


def test_rms_u8_moments_only_and_state_only():
    """batch_mean / batch_var without a state, and a state without them (both are nullable pairs)."""
    import native
    ar = Arena()
    _, x = U8.batch(257, 5)
    xd = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    ws = ar.new(native.rms_u8_workspace_bytes(257, U8.COLS), torch.uint8)
    bmean, bvar = ar.new(U8.COLS, F64), ar.new(U8.COLS, F64)
    native.rms_update_u8(xd, 257, U8.COLS, U8.COLS, None, None, 0.0, ws, bmean, bvar)
    mean, var = ar.new(U8.COLS, F64, init=0.0), ar.new(U8.COLS, F64, init=1.0)
    native.rms_update_u8(xd, 257, U8.COLS, U8.COLS, mean, var, 1e-4, ws)
    ar.check()
    rm = RM.RunningMoments(shape=(U8.COLS,))
    rm.merge(bmean.cpu().numpy(), bvar.cpu().numpy(), 257)
    _bit_equal(mean.cpu().numpy(), rm.mean)
    _bit_equal(var.cpu().numpy(), rm.var)


# ----------------------------------------------------------------- float32 columns
@pytest.mark.parametrize("rows", [1, 2, 1000])
@pytest.mark.parametrize("cols", [2, 255, 257])
def test_rms_f32_columns_strided(cols, rows):
    """One lane per column, rows in numpy's axis-0 order, row_stride = cols + 3; the last block ragged."""
    import native
    ar = Arena()
    rs = np.random.RandomState(cols * 7 + rows)
    mean, var = ar.new(cols, F64, init=0.0), ar.new(cols, F64, init=1.0)
    rm = RM.RunningMoments(shape=(cols,))
    count = 1e-4
    for it in range(3):
        wide = (rs.randn(rows, cols + 3) * 10 ** it + it).astype(np.float32)
        x = wide[:, :cols]
        native.rms_update_f32(torch.from_numpy(wide).cuda(), rows, cols, cols + 3, mean, var, count)
        count += rows
        rm.update(x)
        ar.check()
        _bit_equal(mean.cpu().numpy(), rm.mean, ("mean", it))
        _bit_equal(var.cpu().numpy(), rm.var, ("var", it))


# ----------------------------------------------------------------- scalar float32 streams (numpy's pairwise sums)
SCALAR_N = [9, 128, 129, 136, 1025, 65_537, 262_144]


@pytest.mark.parametrize("n", SCALAR_N)
def test_scalar_pairwise_bitexact(n):
    """ppox_rms_scale_int_rewards (ppo.py:396-398) and ppox_rms_update_f32 with one column: mean, variance and
    the scaled rewards bit for bit numpy's, three updates each, through every leaf shape (the 8-accumulator
    body, its tail, the < 8 loop) and, above 8192 elements, numpy's buffer-sized chunks."""
    import native
    ar = Arena()
    rs = np.random.RandomState(n)
    m1, v1 = ar.new(1, F64, init=0.0), ar.new(1, F64, init=1.0)
    m2, v2 = ar.new(1, F64, init=0.0), ar.new(1, F64, init=1.0)
    rm = RM.RunningMoments()
    count = 1e-4
    for it in range(3):
        ir = (np.abs(rs.randn(n)) * (it + 1) * 1e3).astype(np.float32)
        exp = ir.copy()
        rm.update(exp)
        exp /= (np.sqrt(rm.var) + 1e-08)
        d = ar.new(n, torch.float32, init=ir)
        native.rms_scale_int_rewards(d, m1, v1, count)
        d2 = ar.new(n, torch.float32, init=ir)
        native.rms_update_f32(d2, n, 1, 1, m2, v2, count)
        count += n
        ar.check()
        for m, v in ((m1, v1), (m2, v2)):
            _bit_equal(m.cpu().numpy()[0], rm.mean, ("mean", it))
            _bit_equal(v.cpu().numpy()[0], rm.var, ("var", it))
        _bit_equal(d.cpu().numpy(), exp, ("scaled", it))
        _bit_equal(d2.cpu().numpy(), ir, ("update_f32 leaves its input", it))


def test_scalar_pairwise_refuses_above_its_cap():
    import native
    d = torch.zeros(262_145, device="cuda")
    m, v = torch.zeros(1, dtype=F64, device="cuda"), torch.ones(1, dtype=F64, device="cuda")
    with pytest.raises(native.NativeError, match="ppox_rms_scale_int_rewards: n=262145 unsupported"):
        native.rms_scale_int_rewards(d, m, v, 1e-4)
    with pytest.raises(native.NativeError, match="ppox_rms_update_f32: unsupported 1-col"):
        native.rms_update_f32(d, 262_145, 1, 1, m, v, 1e-4)
    assert float(m) == 0.0 and float(v) == 1.0 and not d.any()


# ----------------------------------------------------------------- VecNormalize rewards, driven directly
VECNORM_MAX_N = 524_288  # 64 full 8192-element chunks of 64 leaves: the largest n the entry point admits


@pytest.mark.parametrize("n", [1, 7, 129, 1025, 65_537, VECNORM_MAX_N])
def test_vecnorm_reward_direct(n):
    """ret, the return moments and the normalised rewards bit for bit oracle/vecnorm.py's arithmetic: update on
    and off, dones given and null, rewards that hit the clip on both sides."""
    import native
    ar = Arena()
    rs = np.random.RandomState(n)
    gamma, eps, clip = 0.99, 1e-8, 1.5
    ref = VecNormalizeNumpy(n, 1, gamma=gamma, epsilon=eps, clip_reward=clip)
    ret = ar.new(n, F64, init=0.0)
    mean, var = ar.new(1, F64, init=0.0), ar.new(1, F64, init=1.0)
    count = 1e-4
    hit = set()
    for step, (update, with_dones) in enumerate([(1, True), (1, False), (0, True), (1, True), (0, False)]):
        rew = (rs.randn(n) * (3.0 + step)).astype(np.float32)
        dones = rs.rand(n) < 0.2
        ref.training = bool(update)
        if update:
            ref._update_reward(rew)
        exp = ref.normalize_reward(rew).astype(np.float32)
        if with_dones:
            ref.ret[dones] = 0
        rd = ar.new(n, torch.float32, init=rew)
        dd = torch.from_numpy(dones.astype(np.uint8)).cuda() if with_dones else None
        native.vecnorm_reward(rd, dd, ret, gamma, mean, var, count, eps, clip, update=update)
        count += n * update
        ar.check()
        got = rd.cpu().numpy()
        _bit_equal(got, exp, ("rewards", step))
        _bit_equal(ret.cpu().numpy(), ref.ret, ("ret", step))
        _bit_equal(mean.cpu().numpy()[0], np.float64(ref.ret_rms.mean), ("mean", step))
        _bit_equal(var.cpu().numpy()[0], np.float64(ref.ret_rms.var), ("var", step))
        hit |= set(np.unique(got[np.abs(got) == np.float32(clip)]).tolist())
    assert n < 100 or hit == {-clip, clip}


def test_vecnorm_reward_refuses_what_overflows_its_leaf_arrays():
    """524,287 elements split into 63 * 64 + 65 leaves, one more than the kernel's arrays hold."""
    import native
    rd = torch.zeros(VECNORM_MAX_N + 1, device="cuda")
    ret = torch.zeros(VECNORM_MAX_N + 1, dtype=F64, device="cuda")
    m, v = torch.zeros(1, dtype=F64, device="cuda"), torch.ones(1, dtype=F64, device="cuda")
    for n in (VECNORM_MAX_N - 1, VECNORM_MAX_N + 1):
        with pytest.raises(native.NativeError, match="pairwise leaves"):
            native.vecnorm_reward(rd[:n], None, ret[:n], 0.99, m, v, 1e-4, 1e-8, 10.0)
    assert float(m) == 0.0 and float(v) == 1.0 and not ret.any()


# ----------------------------------------------------------------- normalize_obs
def _normalize_ref(x, mean, var, eps, clip):
    return np.clip((x - mean) / np.sqrt(var + eps), -clip, clip).astype(np.float32)


@pytest.mark.parametrize("kind,rows,cols", [("u8", 4099, 256), ("f32", 4099, 256), ("ex", 8195, 256),
                                            ("u8", 3, 300), ("f32", 1, 1), ("ex", 5, 7)])
def test_normalize_obs_grid_stride_and_edges(kind, rows, cols):
    """rows * cols just above the grid cap (4096 blocks of 256 for normalize_obs, 8192 for the _ex form), so the
    grid-stride loop takes a second trip; row_stride > cols; values clipped on both edges; columns of zero
    variance.  Bit-exact vs the float64 numpy expression (ppo.py:117; SB3 VecNormalize.normalize_obs)."""
    import native
    assert rows * cols > (8192 if kind == "ex" else 4096) * 256 or rows * cols < 1000
    ar = Arena()
    rs = np.random.RandomState(rows + cols)
    pad = 5
    if kind == "u8":
        wide = rs.randint(0, 256, (rows, cols + pad)).astype(np.uint8)
        mean, var = rs.rand(cols) * 255, rs.rand(cols) * 400 + 1
    else:
        wide = (rs.randn(rows, cols + pad) * 4).astype(np.float32)
        mean, var = rs.randn(cols), rs.rand(cols) + 0.01
    var[::3] = 0.0  # sqrt(eps) alone in the denominator: everything off the mean clips
    x = wide[:, :cols]
    x[:, 0] = x[0, 0]
    mean[0] = np.float64(x[0, 0])  # (x - mean) == 0 over var == 0: 0, not NaN
    eps, clip = (1e-8, 10.0) if kind == "ex" else (1e-10, 5.0)
    exp = _normalize_ref(x, mean, var, eps, clip)
    assert (exp == clip).any() or rows * cols < 10
    assert (exp == -clip).any() or rows * cols < 10
    out = ar.new((rows, cols), torch.float32)
    xd = torch.from_numpy(wide).cuda()
    md, vd = torch.from_numpy(mean).cuda(), torch.from_numpy(var).cuda()
    if kind == "ex":
        native.normalize_obs_f32_ex(xd, rows, cols, cols + pad, md, vd, eps, clip, out)
    else:
        native.normalize_obs(xd, rows, cols, cols + pad, md, vd, out)
    ar.check()
    _bit_equal(out.cpu().numpy(), exp)
    assert not np.isnan(exp).any() and (exp[:, 0] == 0).all()


def test_normalize_obs_no_rows_is_ok():
    import native
    m, v = torch.zeros(7, dtype=F64, device="cuda"), torch.ones(7, dtype=F64, device="cuda")
    for dt in (torch.uint8, torch.float32):
        x = torch.empty(0, 7, dtype=dt, device="cuda")
        native.normalize_obs(x, 0, 7, 7, m, v, torch.empty(0, 7, device="cuda"))
    native.normalize_obs_f32_ex(torch.empty(0, 7, device="cuda"), 0, 7, 7, m, v, 1e-8, 10.0,
                                torch.empty(0, 7, device="cuda"))
    torch.cuda.synchronize()
