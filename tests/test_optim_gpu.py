"""Grad-norm, clip and Adam (csrc/optim.hip) at their tails, grid-stride loops and edge gradients.

References: torch-CPU clip_grad_norm_ + torch.optim.Adam (ppo.py:243-244) at the tolerance of
test_kernels_gpu.py::test_adam_clip_vs_torch, and a float64 restatement of the same update, which bounds what
float32 arithmetic itself costs.  Every buffer a kernel writes is carved out of a sentinel-filled allocation
(tests/guarded.py): the n % 4 tails and the last float4 are exactly where one element too many is written."""
import numpy as np
import pytest
import torch

from guarded import Arena

pytestmark = pytest.mark.gpu

LR, B1, B2, EPS = 3e-4, 0.9, 0.999, 1e-8
# sumsq_kernel strides past 256 blocks x 1024 threads x 4 floats = 1,048,576; adam_kernel past 2048 x 256 float4
SIZES = [1, 3, 5, 4099, 1_048_576 + 7, 2048 * 256 * 4 + 1203]
# torch-f32's own largest |p - p64| over every (n, max_norm) case below after three steps (CPU, measured)
TORCH_F32_DEVIATION = 5.5e-7


def _grads(n, max_norm, steps=3):
    rs = np.random.RandomState(n % 100_003 + int(max_norm * 10) % 97)
    p0 = rs.randn(n).astype(np.float32)
    return p0, [rs.randn(n).astype(np.float32) * (1 + k) for k in range(steps)]


def _f64_norm(g):
    return float(np.sqrt(np.sum(g.astype(np.float64) ** 2)))


# torch-CPU sums a tensor's squares in float32 and falls below the float64 norm by about 1e-11 per element
# (1.0e-5 at 1,048,583 elements in one tensor, 3.6e-5 at 2,098,355; 1e-7 or less up to 16,384).  The flat buffer
# stands for a network's parameter list, so the reference gets it as one: tensors of at most 4099 elements (the
# largest size here that is a single tensor), whose norms torch combines as clip_grad_norm_ does for any model.
REF_TENSOR = 4099


def _torch_reference(p0, grads, max_norm):
    """-> (params, exp_avg, exp_avg_sq, [total norms]) of torch-CPU float32 clip_grad_norm_ + Adam over the
    parameter list p0[0:4099], p0[4099:8198], ..."""
    cuts = list(range(0, len(p0), REF_TENSOR))
    ps = [torch.tensor(p0[o:o + REF_TENSOR], requires_grad=True) for o in cuts]
    opt = torch.optim.Adam(ps, lr=LR, betas=(B1, B2), eps=EPS)
    norms = []
    for g in grads:
        for p, o in zip(ps, cuts):
            p.grad = torch.tensor(g[o:o + REF_TENSOR])
        if max_norm > 0:
            norms.append(float(torch.nn.utils.clip_grad_norm_(ps, max_norm)))
        opt.step()
    cat = lambda ts: torch.cat([t.detach().reshape(-1) for t in ts]).numpy()
    return cat(ps), cat([opt.state[p]["exp_avg"] for p in ps]), cat([opt.state[p]["exp_avg_sq"] for p in ps]), norms


def _f64_reference(p0, grads, max_norm):
    """The same update in float64 (torch/optim/adam.py _single_tensor_adam; clip_grad_norm_'s coefficient)."""
    p = p0.astype(np.float64)
    m, v = np.zeros_like(p), np.zeros_like(p)
    for step, g32 in enumerate(grads, 1):
        g = g32.astype(np.float64)
        if max_norm > 0:
            g = g * min(max_norm / (_f64_norm(g32) + 1e-6), 1.0)
        m = m + (1 - B1) * (g - m)
        v = v * B2 + (1 - B2) * g * g
        bc1, bc2 = 1 - B1 ** step, 1 - B2 ** step
        p = p - (LR / bc1) * (m / (np.sqrt(v) / np.sqrt(bc2) + EPS))
    return p


def _within_one_ulp(got, ref64):
    ref32 = np.float32(ref64)
    return abs(np.float64(got) - np.float64(ref32)) <= np.float64(np.spacing(ref32))


def _device_state(ar, p0):
    import native
    n = len(p0)
    f32 = torch.float32
    p = ar.new(n, f32, init=p0)
    g, m, v = ar.new(n, f32, init=0.0), ar.new(n, f32, init=0.0), ar.new(n, f32, init=0.0)
    part = ar.new(native.NORM_PARTIALS, torch.float64, init=0.0)
    norm = ar.new(1, f32)
    assert all(t.data_ptr() % 16 == 0 for t in (p, g, m, v))  # 16-byte aligned buffers, n itself unpadded
    return p, g, m, v, part, norm


@pytest.mark.parametrize("max_norm", [0.2, 1e9, 0.0])
@pytest.mark.parametrize("n", SIZES)
def test_adam_clip_tails_and_grid_stride(n, max_norm):
    """Three steps at sizes with every n % 4 tail, below one float4, and past both grid-stride thresholds.
    Parameters match torch at rtol 1e-6 / atol 1e-7 and deviate from the float64 restatement by no more than twice
    what torch-f32 itself does.  Measured on the CPU, torch-f32's largest |p - p64| after the three steps is
    1.4e-7 at n = 1 and 3, 1.2e-7 at 5, 2.8e-7 at 4099, 4.8e-7 at 1,048,583 and 5.5e-7 at 2,098,355 (each step
    rounds a parameter of up to |p| = 4.6, whose ulp is 4.8e-7), so the kernel is held to 1.1e-6 (on the
    MI355X its deviation equalled torch's in every case).  total_norm_out is within one float32 ulp of the
    float64 norm; test_total_norm_vs_clip_grad_norm holds it to torch's value."""
    import native
    p0, grads = _grads(n, max_norm)
    tp, tm, tv, tnorms = _torch_reference(p0, grads, max_norm)
    p64 = _f64_reference(p0, grads, max_norm)
    ar = Arena()
    p, g, m, v, part, norm = _device_state(ar, p0)
    for step, gr in enumerate(grads, 1):
        g.copy_(torch.from_numpy(gr))
        if max_norm > 0:
            native.grad_sumsq(g, part)
        native.adam_step(p, g, m, v, part, max_norm, LR, B1, B2, EPS, step, norm_out=norm)
        ar.check()
        assert torch.equal(g.cpu(), torch.from_numpy(gr)), "the step leaves the gradients as they are"
        if max_norm > 0:
            got = norm.cpu().numpy()[0]
            assert _within_one_ulp(got, _f64_norm(gr)), (step, got, _f64_norm(gr))
            np.testing.assert_allclose(float(part.sum()), np.sum(gr.astype(np.float64) ** 2), rtol=1e-13)
    got = p.cpu().numpy()
    np.testing.assert_allclose(got, tp, rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(m.cpu().numpy(), tm, rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(v.cpu().numpy(), tv, rtol=1e-6, atol=1e-7)
    dev_torch = float(np.abs(tp - p64).max())
    dev_kernel = float(np.abs(got - p64).max())
    print(f"n={n} max_norm={max_norm}: |p - p64| torch-f32 {dev_torch:.3e} kernel {dev_kernel:.3e}")
    assert dev_torch <= TORCH_F32_DEVIATION, "the recorded torch-f32 deviation no longer covers torch itself"
    assert dev_kernel <= 2 * TORCH_F32_DEVIATION


@pytest.mark.parametrize("max_norm", [0.2, 1e9])
@pytest.mark.parametrize("n", SIZES)
def test_total_norm_vs_clip_grad_norm(n, max_norm):
    """total_norm_out within rtol 1e-6 of the value torch-CPU float32 clip_grad_norm_ returns for the same
    gradients as a parameter list (_torch_reference), over the three steps.  torch is then within 1.4e-7 of the
    float64 norm at every size, and the kernel within one float32 ulp of it
    (test_adam_clip_tails_and_grid_stride)."""
    import native
    p0, grads = _grads(n, max_norm)
    _, _, _, tnorms = _torch_reference(p0, grads, max_norm)
    ar = Arena()
    p, g, m, v, part, norm = _device_state(ar, p0)
    got = []
    for step, gr in enumerate(grads, 1):
        g.copy_(torch.from_numpy(gr))
        native.grad_sumsq(g, part)
        native.adam_step(p, g, m, v, part, max_norm, LR, B1, B2, EPS, step, norm_out=norm)
        got.append(float(norm))
    ar.check()
    print(f"n={n}: total norms kernel {got} torch {tnorms} float64 {[_f64_norm(gr) for gr in grads]}")
    np.testing.assert_allclose(got, tnorms, rtol=1e-6)


def _ranges(n, kind):
    n4 = n // 4 * 4
    assert n - n4 == 3
    if kind == "whole":
        return [(0, n), (0, 0), (n, 0), (7, 0), (n4, 0)]
    cross = 2048 * 256 * 4 if n > 2048 * 256 * 4 else 1036  # the abutting pair meets where the grid-stride wraps
    return [(5, 6),  # starts and ends inside a float4
            (n4 + 1, 2),  # wholly in the n % 4 tail
            (100, 0),  # empty
            (cross - 37, 37), (cross, 63)]  # abut


@pytest.mark.parametrize("kind", ["mixed", "whole"])
@pytest.mark.parametrize("n", [4099, 2048 * 256 * 4 + 1203])
def test_adam_step_wmax_ranges(n, kind):
    """Per tensor range, the maximum over its slots is max |p| of the new weights in the range bit for bit (0 for
    an empty one), and parameters and moments are bitwise ppox_adam_step's."""
    import native
    rs = np.random.RandomState(n + len(kind))
    p0 = rs.randn(n).astype(np.float32)
    gr = rs.randn(n).astype(np.float32)
    ranges = _ranges(n, kind)
    rt = torch.tensor([lo for lo, _ in ranges] + [c for _, c in ranges], dtype=torch.int64)
    ar = Arena()
    a = _device_state(ar, p0)
    b = _device_state(ar, p0)
    amax = ar.new(native.WMAX_TENSORS * native.WMAX_SLOTS, torch.int32, init=0)
    for step in (1, 2):
        amax.zero_()
        for s in (a, b):
            s[1].copy_(torch.from_numpy(gr * step))
            native.grad_sumsq(s[1], s[4])
        native.adam_step(*a[:5], 0.5, LR, B1, B2, EPS, step, norm_out=a[5])
        native.adam_step_wmax(*b[:5], 0.5, LR, B1, B2, EPS, step, rt, amax, norm_out=b[5])
        ar.check()
        for x, y, name in zip(a, b, ("params", "grads", "exp_avg", "exp_avg_sq", "partials", "norm")):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), (name, step)
        slots = amax.cpu().numpy().view(np.uint32).reshape(native.WMAX_TENSORS, native.WMAX_SLOTS)
        pn = np.abs(b[0].cpu().numpy())
        for t, (lo, c) in enumerate(ranges):
            want = pn[lo:lo + c].max() if c else np.float32(0)
            assert slots[t].max() == want.view(np.uint32), (t, lo, c, slots[t].max().view(np.float32), want)


def test_adam_zero_gradient_with_clipping():
    """An all-zero gradient with clipping on (total norm 0: the coefficient is max_norm / 1e-6 clamped to 1):
    the moments decay and the parameters keep moving, as torch's."""
    import native
    n, max_norm = 4099, 0.5
    p0, grads = _grads(n, max_norm, steps=2)
    grads = [grads[0], np.zeros(n, np.float32), np.zeros(n, np.float32)]
    tp, tm, tv, tnorms = _torch_reference(p0, grads, max_norm)
    ar = Arena()
    p, g, m, v, part, norm = _device_state(ar, p0)
    for step, gr in enumerate(grads, 1):
        g.copy_(torch.from_numpy(gr))
        native.grad_sumsq(g, part)
        native.adam_step(p, g, m, v, part, max_norm, LR, B1, B2, EPS, step, norm_out=norm)
    ar.check()
    assert float(norm) == 0.0 == tnorms[-1]
    assert np.abs(tp - p0).max() > 1.5 * LR  # the zero-gradient steps moved the parameters
    np.testing.assert_allclose(p.cpu().numpy(), tp, rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(m.cpu().numpy(), tm, rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(v.cpu().numpy(), tv, rtol=1e-6, atol=1e-7)


@pytest.mark.parametrize("where", ["first", "tail"])
def test_grad_norm_of_one_huge_element(where):
    """One gradient of 1e18 among zeros (its square, 1e36, needs the float64 accumulator): total_norm_out is the
    float64 norm, and the clipped step is torch's."""
    import native
    n, max_norm = 4099, 0.5
    p0, _ = _grads(n, max_norm, steps=1)
    gr = np.zeros(n, np.float32)
    gr[0 if where == "first" else n - 1] = 1e18
    tp, _, _, tnorms = _torch_reference(p0, [gr], max_norm)
    ar = Arena()
    p, g, m, v, part, norm = _device_state(ar, p0)
    g.copy_(torch.from_numpy(gr))
    native.grad_sumsq(g, part)
    native.adam_step(p, g, m, v, part, max_norm, LR, B1, B2, EPS, 1, norm_out=norm)
    ar.check()
    got = norm.cpu().numpy()[0]
    assert np.isfinite(got) and _within_one_ulp(got, _f64_norm(gr)), (got, _f64_norm(gr))
    np.testing.assert_allclose(got, tnorms[0], rtol=1e-6)
    np.testing.assert_allclose(p.cpu().numpy(), tp, rtol=1e-6, atol=1e-7)
