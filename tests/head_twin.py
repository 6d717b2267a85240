"""References and constructed cases for the action heads of csrc/loss.hip (test helper, not a test
module): f64 twins of the two collect-time samplers, the torch-CPU autograd reference of the fused PPO
loss (Categorical and Box heads, one or two value heads) with a census of the branches it took, and
seeded minibatches whose value heads take a named branch of the max-of-means value loss.
tests/test_head_twin.py checks the twins and the census on the CPU; tests/test_loss_gpu.py and
tests/test_sampler_gpu.py hold the kernels to them."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from oracle import algos as OA
from oracle import philox as PH

F32_EPS = float(np.finfo(np.float32).eps)
M32 = 0xFFFFFFFF
CLASSES = ("pos_above", "pos_below", "neg_above", "neg_below", "inside")
EDGE_REL = 1e-5  # edge_mask: |ratio / (1 +- clip) - 1| < EDGE_REL
EDGE_CAP = 1e-3  # share of a case's rows edge_mask may cover


# ------------------------------------------------------------------------------------------- samplers
def _words(first, n_rows, seed, counter, env_offset):
    """Philox4x32-10 of the samplers' counter {first, env_offset + n, counter lo, counter hi} under the
    key {seed lo, seed hi} (loss.hip categorical_sample_kernel / normal_sample_kernel)."""
    n = ((np.arange(n_rows, dtype=np.int64) + int(env_offset)) & M32).astype(np.uint32)
    counter = int(counter) & 0xFFFFFFFFFFFFFFFF
    return PH.philox4x32_10(np.uint32(first), n, np.uint32(counter & M32), np.uint32(counter >> 32),
                            int(seed) & M32, (int(seed) >> 32) & M32)


def categorical_u(n_rows, seed, counter, env_offset):
    """The uniform (f32, 24 bits) each row's inverse CDF reads."""
    return PH.u01(_words(0xA5A5A5A5, n_rows, seed, counter, env_offset)[0])


def categorical_margin(A):
    """A * 2^-22: the kernel sums at most A f32 probabilities into `cum` (each add rounds by <= 2^-25,
    cum < 1) and each probability comes from an f32 softmax with two normalisations (a few 2^-24
    relative each, the sum of them <= 1), so |cum_f32 - cum_f64| stays below A * 2^-24 + 4 * 2^-24."""
    return A * 2.0 ** -22


def categorical_twin(logits_f32, seed, counter, env_offset, margin):
    """a ~ Categorical(softmax(logits)) by inverse CDF on the kernel's Philox word, in f64.
    Returns (actions int64, log_probs f64, undecidable bool): the action is the number of cumulative
    sums cum_0 .. cum_{A-2} that u has reached (so A - 1 when it has reached all of them); a row is
    undecidable when u lies within `margin` of one of them.  log_prob is log(clamp(q, eps, 1 - eps))
    with the f32 eps, as torch's f32 Categorical(probs=) and the kernel have it."""
    z = np.asarray(logits_f32, np.float32).astype(np.float64)
    N, A = z.shape
    u = categorical_u(N, seed, counter, env_offset).astype(np.float64)
    e = np.exp(z - z.max(1, keepdims=True))
    q = e / e.sum(1, keepdims=True)
    cum = np.cumsum(q, 1)[:, :-1]
    actions = (u[:, None] >= cum).sum(1).astype(np.int64)
    undecidable = (np.abs(u[:, None] - cum) < margin).any(1)
    lp = np.log(np.clip(q[np.arange(N), actions], F32_EPS, 1.0 - F32_EPS))
    return actions, lp, undecidable


def categorical_f32_restatement(logits_f32, u):
    """The kernel's own loop in numpy f32 (categorical.h categorical_forward + the inverse CDF of
    categorical_sample_kernel): sequential f32 sums, e * (1 / S), renormalised q, first j < A - 1 with
    u < cum_j, else A - 1.  np.exp is not expf bit for bit; it is f32-accurate, which is what the
    margin has to cover."""
    z = np.asarray(logits_f32, np.float32)
    N, A = z.shape
    p = np.exp(z - z.max(1, keepdims=True)).astype(np.float32)
    S = np.cumsum(p, 1, dtype=np.float32)[:, -1:]
    p = p * (np.float32(1.0) / S)
    s = np.cumsum(p, 1, dtype=np.float32)[:, -1:]
    q = p / s
    cum = np.cumsum(q, 1, dtype=np.float32)[:, :-1]
    below = np.asarray(u, np.float32)[:, None] < cum
    if A == 1:
        return np.zeros(N, np.int64)
    return np.where(below.any(1), below.argmax(1), A - 1).astype(np.int64)


def normal_twin(mu_f32, log_std_f32, seed, counter, env_offset):
    """a ~ Normal(tanh(mu), exp(log_std)) by Box-Muller on the kernel's Philox words: columns d, d + 1
    (d even) share counter word 0 = 0x5A5A0000 | d; w.x gives u1 (floored at 1e-12), w.y gives u2;
    z_d = r cos(2 pi u2), z_{d+1} = r sin(2 pi u2), r = sqrt(-2 ln u1).  2 pi is the kernel's f32
    constant; everything after the two f32 uniforms is f64.  Returns (actions f64, r f64), both (N, D)."""
    mu = np.asarray(mu_f32, np.float32).astype(np.float64)
    ls = np.asarray(log_std_f32, np.float32).astype(np.float64)
    N, D = mu.shape
    two_pi = np.float64(np.float32(6.283185307179586))
    z, r = np.empty((N, D)), np.empty((N, D))
    for d in range(0, D, 2):
        w = _words(0x5A5A0000 | d, N, seed, counter, env_offset)
        u1 = np.maximum(PH.u01(w[0]), np.float32(1e-12)).astype(np.float64)
        u2 = PH.u01(w[1]).astype(np.float64)
        rad = np.sqrt(-2.0 * np.log(u1))
        z[:, d], r[:, d] = rad * np.cos(two_pi * u2), rad
        if d + 1 < D:
            z[:, d + 1], r[:, d + 1] = rad * np.sin(two_pi * u2), rad
    return np.tanh(mu) + np.exp(ls)[None, :] * z, r


SAMPLER_N, SAMPLER_SEED, SAMPLER_COUNTER = 4099, 2 ** 32 + 5, 3 * 2 ** 32 + 11
SAMPLER_A = (1, 2, 4, 5, 8, 9, 18, 19, 32, 33, 64)
SAMPLER_SCALES = (1.5, 40.0)
UNDECIDABLE_CAP = 0.01


def sampler_logits(N, A, scale):
    """The sampler tests' logits, shared by the CPU margin test and the GPU test."""
    return (np.random.RandomState([N, A, int(scale)]).randn(N, A) * scale).astype(np.float32)


# ---------------------------------------------------------------------------------- value-head cases
def value_case(kind, B, seed, clip):
    """(v, old_v, ret), f32 (B,), for which clipped_value_loss takes a known branch.
    toward: v = ov + sign(ret - ov) * 3 clip rand: the prediction moved toward the return by up to
            3 clip, the clipped one by at most clip, so the clipped mean is the larger;
    away:   the opposite sign: the unclipped mean is the larger;
    tie:    ov, ret multiples of 1/256 in [-2, 2), v = ov + k/256 with |k| <= 64, for clip = 0.25:
            v - ov never leaves the clip range, so vc == v bit for bit, every square is exact in f32
            and the two means are the same number; max() then splits its gradient 0.5 / 0.5, which
            sums to the full gradient because the clamp passes every row."""
    rs = np.random.RandomState(seed)
    if kind == "tie_clipped":
        return _tie_clipped(rs, B, clip)
    if kind == "tie":
        assert clip == 0.25
        ov = rs.randint(-512, 512, B).astype(np.float32) / np.float32(256)
        ret = rs.randint(-512, 512, B).astype(np.float32) / np.float32(256)
        v = ov + rs.randint(-64, 65, B).astype(np.float32) / np.float32(256)
        return v.astype(np.float32), ov, ret
    ov, ret = rs.randn(B).astype(np.float32), rs.randn(B).astype(np.float32)
    step = (np.sign(ret - ov) * np.float32(3 * clip) * rs.rand(B).astype(np.float32)).astype(np.float32)
    assert kind in ("toward", "away")
    return (ov + step if kind == "toward" else ov - step).astype(np.float32), ov, ret


def _tie_clipped(rs, B, clip):
    """A tie in which the clamp matters: everything a multiple of 1/16 (|v - ov| <= 1/4 = clip on the
    plain rows), and B // 4 pairs of rows beyond the clip range whose excesses cancel exactly:
        row i      ret = ov + 3/2 s, v = ov + s/2   (toward, vc = ov + s/4):  e1 - e2 = 1 - 25/16
        row i + 1  ret = ov + 3/4 s, v = ov - s/2   (away,   vc = ov - s/4):  e1 - e2 = 25/16 - 1
    with s = +-1 per pair.  Every square is a multiple of 1/256 below 32 and the sum of B <= 512 of
    them stays below 2^14, so both sums are exact in f32 in any order and the two means are the same
    number although half the rows are clipped.  max() splits 0.5 / 0.5: the clipped rows keep half
    of the unclipped mean's gradient, the others the whole.  Any other pair of tie weights that sums
    to one gives the same gradient on `tie` but not here."""
    assert clip == 0.25 and B <= 512
    q = np.float32(16)
    ov = rs.randint(-32, 32, B).astype(np.float32) / q
    ret = rs.randint(-32, 32, B).astype(np.float32) / q
    v = ov + rs.randint(-4, 5, B).astype(np.float32) / q
    for i in range(0, 2 * (B // 4), 2):
        s = np.float32(rs.choice([-1.0, 1.0]))
        ret[i], v[i] = ov[i] + np.float32(1.5) * s, ov[i] + np.float32(0.5) * s
        ret[i + 1], v[i + 1] = ov[i + 1] + np.float32(0.75) * s, ov[i + 1] - np.float32(0.5) * s
    return v.astype(np.float32), ov, ret


EXPECTED_BRANCH = {"toward": "clipped", "away": "unclipped", "tie": "tie", "tie_clipped": "tie"}


def value_means(v, ov, ret, clip):
    """The two f32 means of clipped_value_loss as torch holds them: (unclipped, clipped)."""
    v, ov, ret = (torch.as_tensor(x) for x in (v, ov, ret))
    vc = ov + (v - ov).clamp(-clip, clip)
    return F.mse_loss(ret, v).item(), F.mse_loss(ret, vc).item()


def _branch(m1, m2):
    return "tie" if m1 == m2 else ("unclipped" if m1 > m2 else "clipped")


# ------------------------------------------------------------------------------------- minibatches
def _clip_of(ext, int_):
    return 0.25 if ext.startswith("tie") or int_.startswith("tie") else 0.2


class Case:
    """One minibatch over a (T, N) rollout: step-major rollout arrays `roll`, env-major flat indices
    `idx` (row b reads element (idx % T) * N + idx // T), the head outputs of its B rows and the
    coefficients.  box: out is mu (B, D) and log_std (D,) is set; else out is logits (B, A)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)
        self._ref = None

    @property
    def elems(self):
        return (self.idx % self.T) * self.N + self.idx // self.T

    def rows(self, name):
        """The minibatch's rows of a rollout array, in minibatch order."""
        a = self.roll[name]
        return a.reshape((self.T * self.N,) + a.shape[2:])[self.elems]

    def reference(self):
        if self._ref is None:
            self._ref = loss_reference(self)
        return self._ref


def _value_heads(rs, roll, t_of, n_of, B, ext, int_, seed, clip):
    v, ov, ret = value_case(ext, B, seed * 7 + 1, clip)
    iv, oiv, iret = value_case(int_, B, seed * 7 + 2, clip)
    for name, x in (("values", ov), ("returns", ret), ("int_values", oiv), ("int_returns", iret)):
        roll[name] = rs.randn(*roll["advantages"].shape).astype(np.float32)
        roll[name][t_of, n_of] = x
    return v, iv


def _finish(kw, roll):
    for a in roll.values():
        a.setflags(write=False)
    return Case(roll=roll, ent_coef=0.01, vf_coef=0.5, int_vf_coef=0.25, scale=0.7, **kw)


@functools.lru_cache(maxsize=None)
def cat_case(T, N, B, A, dual, logit_scale, ext="toward", int_="away", seed=0):
    """Categorical minibatch: logits logit_scale * randn, old log-probs / advantages as
    test_ppo_loss_fwd_bwd_vs_torch draws them, idx the first B of a permutation of T * N, the value
    heads from value_case(ext) and value_case(int_) (clip 0.25 when either is the tie, else 0.2)."""
    rs = np.random.RandomState([T, N, B, A, int(dual), int(logit_scale), seed])
    clip = _clip_of(ext, int_)
    roll = {"actions": rs.randint(0, A, (T, N)).astype(np.int32),
            "log_probs": (np.log(rs.dirichlet(np.ones(A), (T, N))).max(-1) - rs.rand(T, N)).astype(np.float32),
            "advantages": rs.randn(T, N).astype(np.float32) * 2,
            "int_advantages": rs.randn(T, N).astype(np.float32)}
    idx = rs.permutation(T * N)[:B].astype(np.int64)
    v, iv = _value_heads(rs, roll, idx % T, idx // T, B, ext, int_, seed + A, clip)
    out = (rs.randn(B, A) * logit_scale).astype(np.float32)
    return _finish(dict(T=T, N=N, B=B, A=A, D=None, dual=dual, box=False, clip=clip, idx=idx, out=out, values=v,
                        int_values=iv if dual else None, log_std=None, ext=ext, int_=int_), roll)


@functools.lru_cache(maxsize=None)
def box_case(T, N, B, D, dual, ext="toward", int_="away", seed=0):
    """Box minibatch: log_std spans [-3, 1] (shuffled over the D columns), the stored actions are
    draws of the current head and the old log-probs its own log_prob moved by U(-0.5, 0.5), so every
    column's ratios cover both sides of the clip range whatever its scale; its edge_mask is empty by
    construction."""
    rs = np.random.RandomState([T, N, B, D, int(dual), 77, seed])
    clip = _clip_of(ext, int_)
    roll = {"actions": rs.randn(T, N, D).astype(np.float32), "log_probs": -rs.rand(T, N, D).astype(np.float32),
            "advantages": rs.randn(T, N).astype(np.float32) * 2,
            "int_advantages": rs.randn(T, N).astype(np.float32)}
    idx = rs.permutation(T * N)[:B].astype(np.int64)
    t_of, n_of = idx % T, idx // T
    v, iv = _value_heads(rs, roll, t_of, n_of, B, ext, int_, seed + D, clip)
    mu = rs.randn(B, D).astype(np.float32)
    log_std = rs.permutation(np.linspace(-3.0, 1.0, D)).astype(np.float32)
    sc = np.exp(log_std.astype(np.float64))
    act = (np.tanh(mu.astype(np.float64)) + sc * rs.randn(B, D)).astype(np.float32)
    diff = act.astype(np.float64) - np.tanh(mu.astype(np.float64))
    lp = -diff * diff / (2 * sc * sc) - np.log(sc) - 0.5 * np.log(2 * np.pi)
    old = (lp + rs.rand(B, D) - 0.5).astype(np.float32)
    # no element on the surrogate's kink: one whose ratio is within 1e-4 relative of 1 +- clip (ten
    # times the edge band, and far more than this f64 lp differs from the reference's) moves off it
    r = np.exp(lp - old)
    kink = (np.abs(r / (1 + clip) - 1) < 1e-4) | (np.abs(r / (1 - clip) - 1) < 1e-4)
    old[kink] += np.float32(1e-3)
    roll["actions"][t_of, n_of] = act
    roll["log_probs"][t_of, n_of] = old
    return _finish(dict(T=T, N=N, B=B, A=None, D=D, dual=dual, box=True, clip=clip, idx=idx, out=mu, values=v,
                        int_values=iv if dual else None, log_std=log_std, ext=ext, int_=int_), roll)


# (extrinsic, intrinsic) builders of one launch: always different, so a kernel that reads the wrong
# head's branch weights fails; each kind appears on each head once
VALUE_PAIRS = (("toward", "away"), ("away", "tie"), ("tie", "toward"))
TIE_CLIPPED_PAIRS = (("tie_clipped", "away"), ("toward", "tie_clipped"))  # B <= 512 only
BUCKET_A = (1, 2, 5, 8, 9, 18, 19, 32, 33, 64)
BUCKET_SHAPE = (7, 53, 301)      # T, N, B: two blocks of 256 rows, B < T * N
STRIDE_SHAPE = (33, 517, 16641)  # B = 64 * 256 + 257: every thread of the <<<64, 256>>> grid loops
BOX_D = (1, 2, 7, 33, 64)


def bucket_case(A, dual, scale):
    ext, int_ = VALUE_PAIRS[BUCKET_A.index(A) % 3]
    return cat_case(*BUCKET_SHAPE, A, dual, scale, ext, int_)


def box_bucket_case(D, dual):
    ext, int_ = VALUE_PAIRS[BOX_D.index(D) % 3]
    return box_case(*BUCKET_SHAPE, D, dual, ext, int_)


# ---------------------------------------------------------------------------------------- reference
def loss_reference(c, B_global=None):
    """torch-CPU autograd of ppo.py:216-238 (+ the RND terms :431-460) over the whole minibatch `c`,
    with the ops and dtypes of _oracle_loss / test_box_loss_fwd_bwd_vs_torch in tests/test_kernels_gpu.py
    (Categorical: f32 throughout; Box: f64 actions, so f64 log_prob, ratio and surrogate).
    B_global is the row count every mean divides by: the reference is always the one-process
    minibatch, so it must equal c.B; a shard's rows [lo, hi) are compared with rows [lo, hi) of the
    gradients returned here, and its losses with these losses.

    Returns a dict: d_out, dv, div (None unless dual), dls (Box), pl, vl, el, ivl, loss, and
      census     counts of the surrogate classes CLASSES over the rows (Box: over rows x columns),
                 from the f64 ratio and the sign of the normalised advantage;
      vbranch / ivbranch   'unclipped' | 'clipped' | 'tie': the larger of the two f32 means;
      vmeans / ivmeans     those means (unclipped, clipped);
      edge_mask  rows (Box: elements) whose f64 ratio lies within relative EDGE_REL of 1 +- clip,
                 where an f32 log-prob may land on the other side of the surrogate's kink."""
    B_global = c.B if B_global is None else B_global
    assert B_global == c.B, "the reference is the whole minibatch"
    clip = c.clip
    out = torch.tensor(c.out, requires_grad=True)
    v = torch.tensor(c.values, requires_grad=True)
    adv = OA.normalized(torch.tensor(c.rows("advantages")).reshape(-1, 1))
    if c.dual:
        adv = adv + OA.normalized(torch.tensor(c.rows("int_advantages")).reshape(-1, 1))
    ls = None
    if c.box:
        ls = torch.tensor(c.log_std.reshape(1, c.D), requires_grad=True)
        mean = out.tanh()
        dist = torch.distributions.Normal(mean, torch.exp(ls.expand_as(mean)))
        lp = dist.log_prob(torch.tensor(c.rows("actions")).double())
        assert lp.dtype == torch.float64
        old = torch.tensor(c.rows("log_probs"))
    else:
        dist = torch.distributions.Categorical(torch.softmax(out, dim=-1))
        lp = dist.log_prob(torch.tensor(c.rows("actions"), dtype=torch.float64).flatten()).unsqueeze(1)
        old = torch.tensor(c.rows("log_probs")).reshape(-1, 1)
    ratio = torch.exp(lp - old)
    pl = OA.surrogate(adv, ratio, clip)
    ov, ret = torch.tensor(c.rows("values")), torch.tensor(c.rows("returns"))
    vl = OA.clipped_value_loss(ret, v, ov, clip)
    el = -torch.mean(dist.entropy())
    loss = pl + c.ent_coef * el + c.vf_coef * vl
    ivt = ivl = None
    if c.dual:
        ivt = torch.tensor(c.int_values, requires_grad=True)
        ivl = OA.clipped_value_loss(torch.tensor(c.rows("int_returns")), ivt, torch.tensor(c.rows("int_values")), clip)
        loss = loss + c.int_vf_coef * ivl
    (c.scale * loss).backward()
    ref = {"d_out": out.grad.numpy(), "dv": v.grad.numpy(), "div": ivt.grad.numpy() if c.dual else None,
           "dls": ls.grad.numpy()[0] if c.box else None, "pl": pl.item(), "vl": vl.item(), "el": el.item(),
           "ivl": ivl.item() if c.dual else 0.0, "loss": loss.item()}
    # census and edge mask from an f64 ratio
    if c.box:
        r64 = ratio.detach().numpy()
    else:
        z = c.out.astype(np.float64)
        e = np.exp(z - z.max(1, keepdims=True))
        q = np.clip(e[np.arange(c.B), c.rows("actions")] / e.sum(1), F32_EPS, 1.0 - F32_EPS)
        r64 = np.exp(np.log(q) - c.rows("log_probs").astype(np.float64)).reshape(-1, 1)
    a = np.broadcast_to(adv.numpy().astype(np.float64), r64.shape)
    above, below = r64 > 1.0 + clip, r64 < 1.0 - clip
    ref["census"] = {"pos_above": int((above & (a > 0)).sum()), "pos_below": int((below & (a > 0)).sum()),
                     "neg_above": int((above & (a < 0)).sum()), "neg_below": int((below & (a < 0)).sum()),
                     "inside": int((~above & ~below).sum())}
    edge = (np.abs(r64 / (1.0 + clip) - 1.0) < EDGE_REL) | (np.abs(r64 / (1.0 - clip) - 1.0) < EDGE_REL)
    ref["edge_mask"] = edge if c.box else edge[:, 0]
    ref["vmeans"] = value_means(c.values, c.rows("values"), c.rows("returns"), clip)
    ref["vbranch"] = _branch(*ref["vmeans"])
    if c.dual:
        ref["ivmeans"] = value_means(c.int_values, c.rows("int_values"), c.rows("int_returns"), clip)
        ref["ivbranch"] = _branch(*ref["ivmeans"])
    return ref
