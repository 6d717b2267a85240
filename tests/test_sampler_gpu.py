"""The collect-time action heads of csrc/loss.hip (ppox_categorical_sample, its device-counter variant
ppox_categorical_sample_dc, ppox_normal_sample) against the f64 twins of tests/head_twin.py: the same
Philox words, so the same draw on every row the twin can decide, on every action-count bucket; and the
stream identities collect relies on (env_offset sharding, device counter = host counter, both 64-bit
words of counter and seed).  Outputs come out of a sentinel-guarded Arena, NaN / sentinel prefilled."""
import numpy as np
import pytest
import torch

import head_twin as H
from guarded import Arena

pytestmark = pytest.mark.gpu

NAN = float("nan")
N, SEED, COUNTER = H.SAMPLER_N, H.SAMPLER_SEED, H.SAMPLER_COUNTER
UNWRITTEN = -0x5A5A5A5B  # int32 of four sentinel bytes


def up(a):
    return torch.tensor(np.ascontiguousarray(a)).cuda()


def draw(ar, logits, n, A, env_offset, seed, counter, cbase=None):
    """One categorical_sample (or _dc, with a device base) call into fresh guarded outputs, which
    must come back fully written."""
    import native
    acts, lp = ar.new(n, torch.int32), ar.new(n, torch.float32, init=NAN)
    assert (acts == UNWRITTEN).all()
    if cbase is None:
        native.categorical_sample(logits, n, A, env_offset, seed, counter, acts, lp)
    else:
        native.categorical_sample_dc(logits, n, A, env_offset, seed, cbase, counter, acts, lp)
    torch.cuda.synchronize()
    assert not torch.isnan(lp).any() and ((acts >= 0) & (acts < A)).all()
    return acts, lp


def against_twin(z, margin, ar=None):
    """Draw N rows of logits z on the device and compare with categorical_twin: equal actions on every
    decidable row, log-probs of the drawn action at rtol 1e-5 atol 1e-6.  Returns (actions, twin
    actions, undecidable)."""
    own = ar is None
    ar = Arena() if own else ar
    n, A = z.shape
    acts, lp = draw(ar, up(z), n, A, 0, SEED, COUNTER)
    if own:
        ar.check()
    a, lp_t, und = H.categorical_twin(z, SEED, COUNTER, 0, margin)
    got = acts.cpu().numpy().astype(np.int64)
    assert und.mean() <= H.UNDECIDABLE_CAP
    bad = np.flatnonzero((got != a) & ~und)
    assert bad.size == 0, f"{bad.size} decidable rows differ, first {bad[:5]}: got {got[bad[:5]]} twin {a[bad[:5]]}"
    same = got == a
    np.testing.assert_allclose(lp.cpu().numpy()[same], lp_t[same], rtol=1e-5, atol=1e-6)
    # an undecidable row that fell the other way still reports the log-prob of what it drew
    zz = z.astype(np.float64)
    e = np.exp(zz - zz.max(1, keepdims=True))
    q = np.clip(e[np.arange(n), got] / e.sum(1), H.F32_EPS, 1 - H.F32_EPS)
    np.testing.assert_allclose(lp.cpu().numpy(), np.log(q), rtol=1e-5, atol=1e-6)
    return got, a, und


@pytest.mark.parametrize("scale", H.SAMPLER_SCALES)
@pytest.mark.parametrize("A", H.SAMPLER_A)
def test_categorical_sample_is_the_twin(A, scale):
    """N = 4,099 rows (17 blocks, the last with 3 rows) on both sides of every MAXA bucket, plain and
    saturated logits, seed 2^32 + 5 and a counter with a non-zero high word.  Undecidable rows
    (margin A 2^-22) of 4,099 at scale 1.5 / 40: A=18 1/0, 33 4/1, 64 6/0, every other A 0/0."""
    against_twin(H.sampler_logits(N, A, scale), H.categorical_margin(A))


@pytest.mark.parametrize("A", [4, 8, 32, 64])
def test_categorical_sample_equal_logits_every_row(A):
    """All logits equal: q = 1/A and its partial sums are exact in f32, so the action is floor(u A) on
    every row, with no margin and no exclusion."""
    got, a, und = against_twin(np.zeros((N, A), np.float32), 0.0)
    assert not und.any() and np.array_equal(got, a)
    assert np.array_equal(got, np.floor(H.categorical_u(N, SEED, COUNTER, 0).astype(np.float64) * A).astype(np.int64))


@pytest.mark.parametrize("A", [2, 5, 19, 64])
def test_zero_probability_action_is_never_drawn(A):
    """Row n's action n % A has logit -200 against 0: expf underflows, its probability is 0, and it
    is never drawn, whether it is the first, a middle or the last action (the A - 1 fallback)."""
    z = np.zeros((N, A), np.float32)
    z[np.arange(N), np.arange(N) % A] = -200.0
    got, _, _ = against_twin(z, H.categorical_margin(A))
    assert (got != np.arange(N) % A).all()


@pytest.mark.parametrize("A", [1, 2, 5, 33, 64])
def test_fallback_to_the_last_action(A):
    """>= 0.99 of the mass on action A - 1: almost every row runs the inverse CDF to its end without
    u < cum and takes the A - 1 fallback."""
    z = np.zeros((N, A), np.float32)
    z[:, -1] = np.log(200.0 * A)
    e = np.exp(z[0].astype(np.float64))
    assert e[-1] / e.sum() >= 0.99
    got, a, _ = against_twin(z, H.categorical_margin(A))
    assert (got == A - 1).mean() >= 0.98 and (A == 1 or (got != A - 1).any())


# ---------------------------------------------------------------------------------- stream identity
def test_env_offset_shards_are_slices_of_one_stream():
    """Rows [1000, 1300) drawn with env_offset = 1000 are rows 1000.. of one call with offset 0, bit
    for bit (the shard starts inside the fourth block of the whole call and spans two of its own)."""
    k, m, A = 1000, 300, 9
    z = up(H.sampler_logits(k + m, A, 1.5))
    ar = Arena()
    whole = draw(ar, z, k + m, A, 0, SEED, COUNTER)
    part = draw(ar, z[k:], m, A, k, SEED, COUNTER)
    ar.check()
    assert torch.equal(part[0], whole[0][k:]) and torch.equal(part[1], whole[1][k:])
    assert not torch.equal(draw(ar, z[k:], m, A, 0, SEED, COUNTER)[0], whole[0][k:])


@pytest.mark.parametrize("base,off", [(5, 7), (2 ** 32 - 3, 10), (3 * 2 ** 32 + 1, 0)])
def test_device_counter_equals_host_counter(base, off):
    """categorical_sample_dc with device base b and offset o draws what categorical_sample draws with
    counter b + o, including where b + o carries into the high word."""
    A = 18
    z = up(H.sampler_logits(N, A, 1.5))
    ar = Arena()
    cb = up(np.array([base], np.int64))
    dc = draw(ar, z, N, A, 0, SEED, off, cbase=cb)
    host = draw(ar, z, N, A, 0, SEED, base + off)
    ar.check()
    assert torch.equal(dc[0], host[0]) and torch.equal(dc[1], host[1])
    assert int(cb[0]) == base  # the kernel reads the counter, it does not advance it
    other = draw(ar, z, N, A, 0, SEED, off, cbase=up(np.array([base + 1], np.int64)))
    assert not torch.equal(other[0], dc[0])


def test_high_words_of_counter_and_seed_reach_the_stream():
    A = 5
    z = up(H.sampler_logits(N, A, 1.5))
    ar = Arena()
    base = draw(ar, z, N, A, 0, 5, 11)[0]
    assert torch.equal(draw(ar, z, N, A, 0, 5, 11)[0], base)
    for seed, counter in ((5, 11 + 2 ** 32), (5 + 2 ** 32, 11), (5, 12), (6, 11)):
        got = draw(ar, z, N, A, 0, seed, counter)[0]
        assert (got != base).float().mean() > 0.3, (seed, counter)  # independent draws differ on ~ 1 - sum q^2
        twin = H.categorical_twin(z.cpu().numpy(), seed, counter, 0, H.categorical_margin(A))
        assert np.array_equal(got.cpu().numpy()[~twin[2]], twin[0][~twin[2]])
    ar.check()


# -------------------------------------------------------------------------------------- normal head
def _normal_inputs(D):
    rs = np.random.RandomState(D)
    return rs.randn(N, D).astype(np.float32), rs.uniform(-1.0, 0.5, D).astype(np.float32)


@pytest.mark.parametrize("D", [1, 2, 3, 7, 64])
def test_normal_sample_is_the_twin(D):
    """ppox_normal_sample against normal_twin (same Philox words, f64 Box-Muller) on N = 4,099 rows.
    Action tolerance, with sc = exp(log_std), r the Box-Muller radius, a the action:
        atol = sc * 16 * 2^-24 * max(1, r) + 2^-23 * |a|
    z = r cos(t) or r sin(t), t = 2 pi u2 in f32: rounding t (< 2 pi, ulp 2^-21 above 4) moves it by
    <= 4 * 2^-24 absolute, so z by <= 4 * 2^-24 r; cosf / sinf add <= 2 ulp of a value <= 1, i.e.
    <= 2 * 2^-24 r; r = sqrtf(-2 logf(u1)) is off by <= 3 ulp relative, i.e. <= 3 * 2^-24 r |cos| ; the
    product r * cos rounds once more.  That is <= 10 * 2^-24 r; 16 leaves a margin below 2x and
    max(1, r) keeps a floor where r is small.  The last term is the final rounding of loc + sc * z
    (and of loc itself).  log_probs match Normal(loc, sc).log_prob of the returned f32 action at rtol
    1e-5 atol 1e-5, as test_normal_sample_moments_and_logprob has it.  For odd D the pair's unused sine
    must not be stored: the guard behind the last column is checked by Arena.check().
    Measured worst error / tolerance: 0.27, 0.28, 0.30, 0.31, 0.43 for D = 1, 2, 3, 7, 64."""
    import native
    mu, ls = _normal_inputs(D)
    ar = Arena()
    a, lp = ar.new((N, D), torch.float32, init=NAN), ar.new((N, D), torch.float32, init=NAN)
    dmu, dls = up(mu), up(ls)
    native.normal_sample(dmu, dls, N, D, 0, SEED, COUNTER, a, lp)
    ar.check()
    assert not torch.isnan(a).any() and not torch.isnan(lp).any()
    want, r = H.normal_twin(mu, ls, SEED, COUNTER, 0)
    got = a.cpu().numpy().astype(np.float64)
    sc = np.exp(ls.astype(np.float64))[None, :]
    tol = sc * 16 * 2.0 ** -24 * np.maximum(1.0, r) + 2.0 ** -23 * np.abs(want)
    err = np.abs(got - want)
    print(f"D={D}: max err / tol {np.max(err / tol):.3g}")
    assert (err <= tol).all(), f"worst err/tol {np.max(err / tol):.3g} at {np.unravel_index(np.argmax(err / tol), err.shape)}"
    loc, s32 = torch.tanh(dmu).cpu(), torch.exp(dls).cpu()
    ref = torch.distributions.Normal(loc, s32).log_prob(a.cpu())
    np.testing.assert_allclose(lp.cpu().numpy(), ref.numpy(), rtol=1e-5, atol=1e-5)
    # env_offset sharding: rows [1000, 1300) at offset 1000 are rows 1000.. of the whole call
    k, m = 1000, 300
    pa, plp = ar.new((m, D), torch.float32, init=NAN), ar.new((m, D), torch.float32, init=NAN)
    native.normal_sample(dmu[k:k + m].contiguous(), dls, m, D, k, SEED, COUNTER, pa, plp)
    ar.check()
    assert torch.equal(pa, a[k:k + m]) and torch.equal(plp, lp[k:k + m])
    native.normal_sample(dmu[k:k + m].contiguous(), dls, m, D, k, SEED, COUNTER + 2 ** 32, pa, plp)
    torch.cuda.synchronize()
    assert not torch.equal(pa, a[k:k + m])


# ----------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("bad", [0, 65])
def test_samplers_refuse_out_of_range_widths(bad):
    """A (D) = 0 and 65 return an error and launch nothing: the outputs keep their prefill."""
    import native
    n = 8
    ar = Arena()
    z = up(np.zeros((n, 65), np.float32))
    acts, lp = ar.new(n, torch.int32), ar.new(n, torch.float32, init=NAN)
    a, alp = ar.new((n, 65), torch.float32, init=NAN), ar.new((n, 65), torch.float32, init=NAN)
    cb = up(np.array([0], np.int64))
    with pytest.raises(native.NativeError):
        native.categorical_sample(z, n, bad, 0, SEED, COUNTER, acts, lp)
    with pytest.raises(native.NativeError):
        native.categorical_sample_dc(z, n, bad, 0, SEED, cb, 0, acts, lp)
    with pytest.raises(native.NativeError):
        native.normal_sample(z, up(np.zeros(65, np.float32)), n, bad, 0, SEED, COUNTER, a, alp)
    ar.check()
    assert (acts == UNWRITTEN).all() and torch.isnan(lp).all() and torch.isnan(a).all() and torch.isnan(alp).all()
