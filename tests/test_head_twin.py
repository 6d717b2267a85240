"""tests/head_twin.py on the CPU: the sampler twins against torch and against an f32 restatement of the
kernel's loop, and the conditions the GPU tests of csrc/loss.hip rely on (every surrogate class
present, the edge mask small, each value-head builder on the branch it is named for), asserted on the
reference alone."""
import numpy as np
import pytest
import torch

import head_twin as H


# ------------------------------------------------------------------------------------------ samplers
def test_categorical_twin_logprob_and_frequencies():
    """log-probs are torch's f64 Categorical(probs=softmax) up to the f32 eps clamp (2^-23 absolute);
    frequencies over 200,000 rows of one distribution match its probabilities (4e-3: 3.6 sigma of the
    largest binomial std 1.1e-3, the bound test_categorical_sample_distribution uses)."""
    N, A = 200_000, 4
    row = np.array([0.0, 1.0, 2.0, -1.0], np.float32)
    logits = np.repeat(row[None], N, 0)
    a, lp, und = H.categorical_twin(logits, 1234, 7, 0, H.categorical_margin(A))
    p = torch.softmax(torch.tensor(row, dtype=torch.float64), -1)
    np.testing.assert_allclose(np.bincount(a, minlength=A) / N, p.numpy(), atol=4e-3)
    ref = torch.distributions.Categorical(probs=p).log_prob(torch.as_tensor(a)).numpy()
    np.testing.assert_allclose(lp, ref, rtol=1e-12, atol=2.0 ** -23)
    assert und.mean() <= H.UNDECIDABLE_CAP
    rs = np.random.RandomState(0)
    z = (rs.randn(1000, 9) * 1.5).astype(np.float32)
    a, lp, _ = H.categorical_twin(z, 5, 6, 7, H.categorical_margin(9))
    d = torch.distributions.Categorical(probs=torch.softmax(torch.tensor(z, dtype=torch.float64), -1))
    np.testing.assert_allclose(lp, d.log_prob(torch.as_tensor(a)).numpy(), rtol=1e-12, atol=2.0 ** -23)


@pytest.mark.parametrize("A", [4, 8, 32, 64])
def test_categorical_twin_equal_logits_is_floor_u_A(A):
    """q = 1/A and its cumulative sums are exact, u has 24 bits: the action is floor(u * A) on every
    row and, with margin 0, no row is undecidable unless u sits on a multiple of 1/A (then u >= cum
    decides it, the same way in f32).  The GPU test's zero-exclusion case."""
    N = H.SAMPLER_N
    a, lp, und = H.categorical_twin(np.zeros((N, A), np.float32), H.SAMPLER_SEED, H.SAMPLER_COUNTER, 0, 0.0)
    u = H.categorical_u(N, H.SAMPLER_SEED, H.SAMPLER_COUNTER, 0)
    assert np.array_equal(a, np.floor(u.astype(np.float64) * A).astype(np.int64))
    assert not und.any()
    assert len(np.unique(a)) == A
    np.testing.assert_allclose(lp, -np.log(A), rtol=1e-15)
    assert np.array_equal(H.categorical_f32_restatement(np.zeros((N, A), np.float32), u), a)


@pytest.mark.parametrize("scale", H.SAMPLER_SCALES)
@pytest.mark.parametrize("A", H.SAMPLER_A)
def test_undecidable_share_and_f32_restatement(A, scale):
    """margin = A * 2^-22 leaves at most 1 % of the GPU sampler test's rows undecidable, and an f32
    restatement of the kernel's loop agrees with the f64 twin on every decidable row.  Measured
    undecidable rows of 4,099, scale 1.5 / 40:  A=18 1/0, A=33 4/1, A=64 6/0, every other A 0/0 (worst
    0.15 %)."""
    z = H.sampler_logits(H.SAMPLER_N, A, scale)
    a, _, und = H.categorical_twin(z, H.SAMPLER_SEED, H.SAMPLER_COUNTER, 0, H.categorical_margin(A))
    print(f"A={A} scale={scale}: undecidable {int(und.sum())} of {len(und)}")
    assert und.mean() <= H.UNDECIDABLE_CAP
    a32 = H.categorical_f32_restatement(z, H.categorical_u(H.SAMPLER_N, H.SAMPLER_SEED, H.SAMPLER_COUNTER, 0))
    assert np.array_equal(a32[~und], a[~und])


def test_sampler_words_shard_and_counter():
    """The twin's own stream identities: rows [k, k + m) at env_offset k are rows k.. at offset 0; the
    high counter word and the high seed word both change the draw."""
    u0 = H.categorical_u(1300, H.SAMPLER_SEED, 7, 0)
    assert np.array_equal(H.categorical_u(300, H.SAMPLER_SEED, 7, 1000), u0[1000:])
    assert not np.array_equal(H.categorical_u(1300, H.SAMPLER_SEED, 7 + 2 ** 32, 0), u0)
    assert not np.array_equal(H.categorical_u(1300, H.SAMPLER_SEED + 2 ** 32, 7, 0), u0)


def test_normal_twin_moments_and_pairing():
    """Box-Muller columns are standard normal (mean within 4 sigma, std within 2 %), columns d, d + 1
    share a radius, and an odd D drops the last sine."""
    N, D = 100_000, 3
    mu, ls = np.zeros((N, D), np.float32), np.zeros(D, np.float32)
    a, r = H.normal_twin(mu, ls, 99, 5, 0)
    np.testing.assert_allclose(a.mean(0), 0.0, atol=4 / np.sqrt(N))
    np.testing.assert_allclose(a.std(0), 1.0, rtol=2e-2)
    assert np.array_equal(r[:, 0], r[:, 1]) and not np.array_equal(r[:, 0], r[:, 2])
    np.testing.assert_allclose(a[:, 0] ** 2 + a[:, 1] ** 2, r[:, 0] ** 2, rtol=1e-12)
    a4, _ = H.normal_twin(np.zeros((N, 4), np.float32), np.zeros(4, np.float32), 99, 5, 0)
    assert np.array_equal(a4[:, :3], a)


# ---------------------------------------------------------------------------------- value-head cases
@pytest.mark.parametrize("kind", ["toward", "away", "tie"])
@pytest.mark.parametrize("B", [301, 16641])
def test_value_case_takes_its_branch(kind, B):
    """toward / away: the two means differ by more than 1 % relative, on the named side; tie: they are
    bit-equal and torch's max() backward then equals the full gradient of either mean.  Measured at
    B = 16,641 (unclipped / clipped): toward 1.451 / 1.664, away 2.808 / 2.416."""
    clip = 0.25 if kind == "tie" else 0.2
    for seed in (1, 2):  # the extrinsic and the intrinsic head draw independent sets
        v, ov, ret = H.value_case(kind, B, seed, clip)
        m1, m2 = H.value_means(v, ov, ret, clip)
        print(f"{kind} B={B} seed={seed}: unclipped {m1:.6g} clipped {m2:.6g}")
        assert H._branch(m1, m2) == H.EXPECTED_BRANCH[kind]
        if kind == "tie":
            assert m1 == m2
            vt = torch.tensor(v, requires_grad=True)
            H.OA.clipped_value_loss(torch.tensor(ret), vt, torch.tensor(ov), clip).backward()
            full = torch.tensor(v, requires_grad=True)
            H.F.mse_loss(torch.tensor(ret), full).backward()
            assert torch.equal(vt.grad, full.grad)
        else:
            assert abs(m1 - m2) > 0.01 * max(m1, m2)


def test_tie_clipped_is_a_tie_with_clipped_rows():
    """tie_clipped: bit-equal means with half the rows outside the clip range; torch's max() backward
    leaves those rows half the unclipped gradient and the others the whole of it."""
    B, clip = 301, 0.25
    for seed in (1, 2):
        v, ov, ret = H.value_case("tie_clipped", B, seed, clip)
        m1, m2 = H.value_means(v, ov, ret, clip)
        assert m1 == m2
        clipped = np.abs(v - ov) > clip
        assert clipped.sum() == 2 * (B // 4)
        vt = torch.tensor(v, requires_grad=True)
        H.OA.clipped_value_loss(torch.tensor(ret), vt, torch.tensor(ov), clip).backward()
        full = -2.0 * (ret.astype(np.float64) - v) / B
        np.testing.assert_allclose(vt.grad.numpy()[~clipped], full[~clipped], rtol=1e-6)
        np.testing.assert_allclose(vt.grad.numpy()[clipped], 0.5 * full[clipped], rtol=1e-6)
        assert np.abs(full[clipped]).min() > 0


# ------------------------------------------------------------------------------------------- census
def _check_census(c, min_rows):
    ref = c.reference()
    n = ref["edge_mask"].size
    print(f"T={c.T} N={c.N} B={c.B} A={c.A} D={c.D} dual={c.dual}: census {ref['census']} "
          f"edge {int(ref['edge_mask'].sum())} of {n}; v {ref['vbranch']} {ref['vmeans']}")
    assert sum(ref["census"].values()) == n
    assert all(ref["census"][k] >= min_rows for k in H.CLASSES)
    assert ref["edge_mask"].mean() <= H.EDGE_CAP
    assert ref["vbranch"] == H.EXPECTED_BRANCH[c.ext]
    if c.dual:
        assert ref["ivbranch"] == H.EXPECTED_BRANCH[c.int_]


def test_census_of_the_grid_stride_case():
    """(T, N, B, A) = (33, 517, 16641, 5), logits 1.5 randn, clip 0.2: every surrogate class has at
    least 100 rows and the edge mask covers at most 0.1 % of them.  Measured: pos_above 1,842,
    pos_below 5,667, neg_above 1,905, neg_below 5,597, inside 1,630; edge 0 of 16,641."""
    c = H.cat_case(33, 517, 16641, 5, True, 1.5)
    _check_census(c, 100)
    assert c.reference()["div"] is not None
    # the other grid-stride cases of the GPU test: 0 edge rows each
    for T, N, B, A, dual in ((33, 517, 16641, 64, True), (33, 517, 16385, 5, False), (33, 517, 16385, 18, True)):
        _check_census(H.cat_case(T, N, B, A, dual, 1.5), 100)


def test_census_of_the_box_case():
    """Box head, D = 3 at B = 16641: the classes are counted over rows x columns.  Measured:
    pos_above 8,029, pos_below 6,855, neg_above 7,863, neg_below 6,851, inside 20,325; edge 0 of 49,923."""
    _check_census(H.box_case(33, 517, 16641, 3, True), 100)


def test_every_small_gpu_case_meets_its_conditions():
    """The B = 301 cases of tests/test_loss_gpu.py (every action bucket x one / two value heads x both
    logit scales, every Box width): the value heads take the named branches and the edge mask is
    within its cap, which at 301 rows means empty.  Measured: 0 edge rows in every case."""
    cases = [H.bucket_case(A, dual, s) for A in H.BUCKET_A for dual in (False, True) for s in (1.5, 40.0)]
    cases += [H.box_bucket_case(D, dual) for D in H.BOX_D for dual in (False, True)]
    cases += [H.cat_case(*H.BUCKET_SHAPE, 5, dual, 1.5, e, i) for e, i in H.VALUE_PAIRS for dual in (False, True)]
    cases += [H.box_case(*H.BUCKET_SHAPE, 3, dual, e, i) for e, i in H.VALUE_PAIRS for dual in (False, True)]
    cases += [H.cat_case(*H.BUCKET_SHAPE, 5, dual, 1.5, e, i) for e, i in H.TIE_CLIPPED_PAIRS for dual in (False, True)]
    cases += [H.box_case(*H.BUCKET_SHAPE, 3, dual, e, i) for e, i in H.TIE_CLIPPED_PAIRS for dual in (False, True)]
    cases += [H.box_case(*H.BUCKET_SHAPE, 7, dual) for dual in (False, True)]
    cases += [H.box_case(*H.BUCKET_SHAPE, 2, True, "toward", "away"), H.cat_case(*H.BUCKET_SHAPE, 9, True, 40.0, "away", "tie")]
    for c in cases:
        ref = c.reference()
        assert ref["edge_mask"].mean() <= H.EDGE_CAP, (c.A, c.D, c.dual, ref["edge_mask"].sum())
        assert ref["vbranch"] == H.EXPECTED_BRANCH[c.ext]
        if c.dual:
            assert ref["ivbranch"] == H.EXPECTED_BRANCH[c.int_]
        assert np.isfinite(ref["d_out"]).all() and np.isfinite(ref["loss"])
        if c.A == 1:
            assert not ref["d_out"].any()  # one action: the policy has no gradient, exactly


def test_reference_gradient_is_zero_outside_the_clip_range():
    """The census classes mean what the GPU test takes them to mean: with ent_coef = 0, rows of class
    pos_above and neg_below have no policy gradient, every other class has one."""
    c = H.cat_case(7, 53, 301, 5, False, 1.5)
    c0 = H.Case(**{k: v for k, v in c.__dict__.items() if k != "_ref"})
    c0.ent_coef = 0.0
    ref = H.loss_reference(c0)
    z = c0.out.astype(np.float64)
    q = np.exp(z - z.max(1, keepdims=True))
    q = q[np.arange(c0.B), c0.rows("actions")] / q.sum(1)
    r = np.exp(np.log(q) - c0.rows("log_probs"))
    adv = c0.rows("advantages").astype(np.float64)
    adv = adv - adv.mean()
    dead = ((adv > 0) & (r > 1 + c0.clip)) | ((adv < 0) & (r < 1 - c0.clip))
    assert dead.sum() > 30 and (~dead).sum() > 30
    assert not ref["d_out"][dead].any() and np.abs(ref["d_out"][~dead]).max(1).min() > 0
