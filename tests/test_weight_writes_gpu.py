"""The packed weight forms follow every write to the weights ("Writes to the weights").

The split-f16 hot path never reads the f32 weights: it reads forms derived from them (NatureConvs.pack's f16 planes
q*, qfc, qh, the f32 packings wp* / wpd*, wfc_nhwc, their tails with the H1P exponent, the PX norms and the bias
bounds; NativeIcm.pack's W1 planes) and the packing may take its amax from the Adam step (convs.WmaxLink).  Every
kernel is held to float64 elsewhere in the suite; here the kernels must be handed the CURRENT weights: after a write
by any route, from any cache state, a pass must be bitwise the pass of a freshly built net and trunk holding the new
weights (the kernels are deterministic across instances: test_wmax_fold_gpu.test_training_steps_fold_on_off_bitwise),
and stay within the float64 bound of tests/test_px_gpu.py.

Routes: writes through torch (load_state_dict, an in-place op on a Parameter or on the flat buffer) move a version
counter and are followed with no call from the writer; x.data.copy_() and a native kernel on the raw buffer move none
and are announced by FlatParams.touch().  States before the write: one pass (the pure stale cache), one pass and an
optimizer step (the Adam-amax fold armed), and those plus a pass at another form set (a later pass must not mix two
generations of weights).  New weights: an independent re-init; the old weights with the fc and conv1 weights x 8 (a
stale exponent overflows the f16 planes: amax is scaled into [2^14, 2^15) and 8 x 2^14 > 65504) and x 2^-12 (a
stale exponent loses the low plane).  Each case first shows on the float64 reference alone that it can tell the old
weights from the new: max |logits(new) - logits(old)| >= 0.1 max |logits(new)|.

Reference: the layer math of models-checkpoint.py:48-90 in float64 (test_px_gpu._fp64_masked), and the project's own
fresh build as the bitwise oracle."""
import pytest
import torch

import test_px_gpu as PX

pytestmark = pytest.mark.gpu

A, B = 6, 37  # a ragged tile, more than one workgroup
SEED_OLD, SEED_NEW = 21, 22
ROUTES = ("load_state_dict", "param_copy", "flat_copy", "data_copy+touch", "native+touch")
STATES = ("pass", "step", "step_forms")
KINDS = ("reinit", "x8", "x2m12")  # x2m12: x 2^-12

_cache = {}


def _once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _inputs():
    def make():
        g = torch.Generator(device="cuda").manual_seed(5)
        x = torch.randint(0, 256, (B, 4, 84, 84), dtype=torch.uint8, device="cuda", generator=g)
        return x, torch.randn(B, A, device="cuda", generator=g), torch.randn(B, device="cuda", generator=g)
    return _once("inputs", make)


def _init_sd(seed):
    """a CnnActorCritic's initial weights from a torch seed (CPU, never written)"""
    def make():
        import models
        torch.manual_seed(seed)
        return {k: v.clone() for k, v in models.CnnActorCritic(4, A).state_dict().items()}
    return _once(("init", seed), make)


def _build(sd, math):
    """the weights written into a new CnnActorCritic before FlatParams and attach"""
    import convs
    import models
    net = models.CnnActorCritic(4, A)
    net.load_state_dict(sd)
    flat = models.FlatParams(net, "cuda")
    cv = convs.attach(net, flat, math)
    return net, flat, cv


def _weights(net):
    return {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}


def _forms(cv):
    """form name (NatureConvs._forms) -> its buffer"""
    d = {"wp1": cv.wp1, "wp2": cv.wp2, "wp3": cv.wp3, "wpd2": cv.wpd2, "wpd3": cv.wpd3, "q1": cv.q[1], "q2": cv.q[2],
         "q3": cv.q[3], "qd2": cv.q[12], "qd3": cv.q[13]}
    if cv.qfc is not None:
        d.update(qfcf=cv.qfc[0], qfcd=cv.qfc[1], qhf=cv.qh[0], qhd=cv.qh[1], wfc_nhwc=cv.wfc_nhwc)
    return d


def _train_pass(net, flat, cv):
    """the explicit training pass: (logits, values, parameter gradients, the pass's ReLU masks, packed forms)"""
    x, dout, dv = _inputs()
    flat.zero_grad()
    out, v, _, ctx = net.forward_train(x)
    net.backward_train(ctx, dout, dv)
    torch.cuda.synchronize()
    grads = {n: p.grad.detach().clone() for n, p in net.named_parameters()}
    bufs = _forms(cv)
    packed = {name: bufs[name].clone() for name in sorted(cv._packed)}
    return out.detach().clone(), v.detach().clone(), grads, PX._relu_masks(ctx), packed


def _ref64(sd):
    import models
    ref = models.CnnActorCritic(4, A)
    ref.load_state_dict(sd)
    return ref.double()


def _logits64(sd):
    """float64 logits of the reference architecture with weights sd (its own ReLU decisions)"""
    x, dout, dv = _inputs()
    return PX._fp64(_ref64(sd), x, dout, dv)[0]


def _ref64_masked(sd, masks):
    """float64 outputs and gradients with weights sd and a pass's own ReLU masks"""
    x, dout, dv = _inputs()
    return PX._fp64_masked(_ref64(sd), x, dout, dv, masks)


def _errors(ref, res):
    """each output's error against the float64 reference, normalised as tests/test_px_gpu.py does"""
    out, v, grads, _, _ = res
    r_out, r_v, r_g = ref
    errs = {}
    for name, a, r in [("out", out, r_out), ("v", v, r_v)] + [(n, grads[n], r_g[n]) for n in r_g]:
        errs[name] = (a.cpu().double() - r).abs().max().item() / (r.abs().max().item() + 1e-30)
    return errs


def _same_sd(a, b):
    return a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)


def _same_form(name, x, y):
    """two instances' packings of one form, bit for bit in every word a packer writes (as test_wmax_fold_gpu._same,
    which compares two packings into ONE buffer and so may compare the whole tail: across instances the words no
    packer writes are the allocations' own bytes).  csrc/conv_common.h: the planes; the tail's amax partials, which
    only the packer reads, by their maximum; the exponent; q1's H1P exponent; the bias bound and the 256 column-norm
    partials of the forms that bound a PX output (q2, q3, qd3, qfcd).  f32 forms: every word."""
    import native
    if x.dtype != torch.int16:
        return torch.equal(x.view(torch.int32), y.view(torch.int32))
    S = native.AMAX_SLOTS
    t0 = x.numel() - 2 * native.PACK_TAIL32
    tx, ty = x[t0:].view(torch.int32), y[t0:].view(torch.int32)
    words = [S] + ([S + 1] if name == "q1" else [])
    if name in ("q2", "q3", "qd3", "qfcd"):
        words += [S + 2] + list(range(S + 8, 2 * S + 8))
    words = torch.tensor(words, device=x.device)
    return (torch.equal(x[:t0], y[:t0]) and int(tx[:S].max()) == int(ty[:S].max())  # (non-negative float bits)
            and torch.equal(tx[words], ty[words]))


def _same_masks(a, b):
    return all((x is None and y is None) or (x is not None and y is not None and torch.equal(x, y)) for x, y in zip(a, b))


def _oracle(key, W, math):
    """the fresh build's pass with weights W, its float64 reference and errors, computed once per distinct W and
    settings"""
    def make():
        net, flat, cv = _build(W, math)
        res = _train_pass(net, flat, cv)
        ref = _ref64_masked(W, res[3])
        return W, res, ref, _errors(ref, res), _logits64(W)
    got = _once(("oracle",) + key, make)
    assert _same_sd(got[0], W), "the cases sharing this oracle wrote the same weights"
    return got[1:]


def _target(kind, old):
    if kind == "reinit":
        return {k: v.clone() for k, v in _init_sd(SEED_NEW).items()}
    s = 8.0 if kind == "x8" else 2.0 ** -12
    new = {k: v.clone() for k, v in old.items()}
    for k in ("feature_extractor.7.weight", "feature_extractor.0.weight"):
        new[k] = new[k] * s
    return new


def _flat_of(net, flat, sd):
    """sd laid out as the flat buffer (the order of FlatParams.params), on the device"""
    by_ptr = {p.data_ptr(): n for n, p in net.named_parameters()}
    return torch.cat([sd[by_ptr[p.data_ptr()]].reshape(-1) for p in flat.params]).cuda()


def _versions(net, flat):
    return (flat.data._version,) + tuple(p._version for p in net.parameters())


def _native_write(net, flat, target):
    """ppox_adam_step called directly on the flat buffer (not FlatParams.adam_step: no step count moves), with a
    gradient, lr and eps chosen so that its first step moves every weight to ~target: update = lr g / (|g| + eps)
    = g (1 - O(|g| / eps)) with g = w - target and lr = eps = 2^30.  What it wrote is read back as the new weights."""
    import native
    n = flat.data.numel()
    g = torch.zeros(n, device="cuda")
    g[:flat.n] = flat.data[:flat.n] - _flat_of(net, flat, target)
    m, v = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    native.adam_step(flat.data, g, m, v, flat.norm_partials, 0.0, 2.0 ** 30, 0.9, 0.999, 2.0 ** 30, 1)


def _write(route, net, flat, target):
    if route == "load_state_dict":
        net.load_state_dict(target)
    elif route == "param_copy":
        with torch.no_grad():
            for n, p in net.named_parameters():
                p.copy_(target[n])
    elif route == "flat_copy":
        flat.data[:flat.n].copy_(_flat_of(net, flat, target))
    elif route.startswith("data_copy"):
        for n, p in net.named_parameters():
            p.data.copy_(target[n])
    elif route.startswith("native"):
        _native_write(net, flat, target)
    else:
        raise ValueError(route)
    if route.endswith("+touch"):
        flat.touch()


def _prepare(state, net, flat, cv, monkeypatch):
    """the cache state before the write; returns the form set of the default pass"""
    import convs
    _train_pass(net, flat, cv)
    forms1 = set(cv._packed)
    assert forms1 == cv._forms(B)
    if state == "pass":
        return forms1
    flat.adam_step(2.5e-4, 0.5)
    assert cv._wmax.valid is not None, "the fold is armed"
    if state == "step_forms":
        # a pass at another form set: the heads' hidden layer on the large-batch kernels (as test_product_gpu's
        # head_min = 0) — which at this batch reads the same two forms — and the fc forward on the library GEMM,
        # which reads wfc_nhwc instead of qfcf: the default pass after the write then finds qfcf missing
        with monkeypatch.context() as m:
            m.setattr(convs, "HEAD_SPLIT_MIN_BATCH", 0)
            m.setattr(convs, "FC_SPLIT_MIN_BATCH", B + 1)
            forms2 = cv._forms(B)
            assert forms2 != forms1 and "wfc_nhwc" in forms2 and "qfcf" not in forms2
            _train_pass(net, flat, cv)
            assert cv._packed == forms2
    return forms1


def _case(route, state, kind, math, monkeypatch, tag=()):
    monkeypatch.setenv("PPOX_WMAX_FOLD", "1")
    net, flat, cv = _build(_init_sd(SEED_OLD), math)
    forms1 = _prepare(state, net, flat, cv, monkeypatch)
    old = _weights(net)
    target = _target(kind, old)
    _write(route, net, flat, target)
    W = _weights(net)  # (reads the weights: no cache is touched)
    if not route.startswith("native"):
        assert _same_sd(W, target)
    key = (math, state != "pass", kind, route.startswith("native")) + tuple(tag)
    o_res, o_ref, o_err, l_new = _oracle(key, W, math)
    # the case can tell stale from fresh, on the float64 reference alone
    l_old = _once(("logits_old", state != "pass"), lambda: (old, _logits64(old)))
    assert _same_sd(l_old[0], old)
    gap, top = (l_new - l_old[1]).abs().max().item(), l_new.abs().max().item()
    print(f"float64 logits: max|new - old| = {gap:.4g}, max|new| = {top:.4g}")
    assert gap >= 0.1 * top
    res = _train_pass(net, flat, cv)
    out, v, grads, masks, packed = res
    o_out, o_v, o_grads, o_masks, o_packed = o_res
    bad = [n for n, t in [("out", out), ("v", v)] + list(grads.items()) if not torch.isfinite(t).all()]
    assert not bad, f"non-finite: {bad}"
    # float64, with the pass's own ReLU decisions (the oracle's reference is that one when the masks are the same)
    errs = _errors(o_ref if _same_masks(masks, o_masks) else _ref64_masked(W, masks), res)
    over = {n: (errs[n], o_err[n]) for n in errs if not errs[n] <= 2 * o_err[n] + 2e-7}
    print("worst error vs float64 (case, fresh):", max((errs[n], o_err[n], n) for n in errs))
    assert not over, over
    # bitwise the fresh build's pass
    assert torch.equal(out.view(torch.int32), o_out.view(torch.int32)), "logits"
    assert torch.equal(v.view(torch.int32), o_v.view(torch.int32)), "values"
    diff = [n for n in o_grads if not torch.equal(grads[n].view(torch.int32), o_grads[n].view(torch.int32))]
    assert not diff, f"gradients differ: {diff}"
    assert set(packed) == set(o_packed) == forms1
    diff = [n for n in o_packed if not _same_form(n, packed[n], o_packed[n])]
    assert not diff, f"packed forms differ: {diff}"
    return forms1


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("state", STATES)
@pytest.mark.parametrize("route", ROUTES)
def test_pass_after_a_weight_write_is_the_fresh_builds(route, state, kind, monkeypatch):
    _case(route, state, kind, "split", monkeypatch)


@pytest.mark.parametrize("math", ["f32", "split_all"])
@pytest.mark.parametrize("route", ["load_state_dict", "flat_copy"])
def test_pass_after_a_weight_write_other_math_modes(route, math, monkeypatch):
    """the f32 packings wp* / wpd* (f32 math) and every split kernel (split_all)"""
    _case(route, "pass", "reinit", math, monkeypatch)


@pytest.mark.parametrize("route", ["load_state_dict", "flat_copy"])
def test_pass_after_a_weight_write_library_fc_forward(route, monkeypatch):
    """the fc forward on the library GEMM reads wfc_nhwc, a permuted f32 copy of the weight"""
    import convs
    monkeypatch.setattr(convs, "FC_SPLIT_MIN_BATCH", B + 1)
    forms = _case(route, "pass", "reinit", "split", monkeypatch, tag=("wfc_nhwc",))
    assert "wfc_nhwc" in forms and "qfcf" not in forms


@pytest.mark.parametrize("route", ["data_copy", "native"])
def test_counterless_write_moves_no_torch_counter(route, monkeypatch):
    """why FlatParams.touch() exists: x.data.copy_() and a native kernel on the raw buffer change the weights and
    move neither the flat buffer's version counter nor any Parameter's, so no key can follow them"""
    net, flat, cv = _build(_init_sd(SEED_OLD), "split")
    _train_pass(net, flat, cv)
    old = _weights(net)
    versions, key = _versions(net, flat), cv.weights_key()
    _write(route, net, flat, _target("reinit", old))
    torch.cuda.synchronize()
    assert not _same_sd(_weights(net), old), "the weights did change"
    assert _versions(net, flat) == versions and cv.weights_key() == key
    flat.touch()
    assert cv.weights_key() != key


# ---- the ICM encoder's W1 planes (NativeIcm.pack), consumer: NativeIcm.encode
K_ICM, A_ICM, M_ICM = 4 * 84 * 84, 4, 33


def _icm_module(seed):
    from env import Discrete
    from models import IntrinsicCuriosityModule
    from util import ActionConverter
    torch.manual_seed(seed)
    return IntrinsicCuriosityModule(K_ICM, ActionConverter(Discrete(A_ICM)), 32)


def _icm_native(module):
    import icm as icm_native
    from models import FlatParams
    flat = FlatParams(module, "cuda")
    assert icm_native.supported(module, flat, (K_ICM,), torch.uint8)
    return flat, icm_native.NativeIcm(module, flat, K_ICM)


def _icm_frames():
    def make():
        g = torch.Generator().manual_seed(9)
        return torch.randint(0, 256, (M_ICM, K_ICM), dtype=torch.uint8, generator=g)
    return _once("icm_frames", make)


def _phi64(sd):
    ref = _icm_module(0)
    ref.load_state_dict(sd)
    with torch.no_grad():
        return ref.double().state_encoder(_icm_frames().double())


@pytest.mark.parametrize("stepped", [False, True])
@pytest.mark.parametrize("route", ["load_state_dict", "flat_copy", "data_copy+touch"])
def test_icm_encode_after_a_weight_write(route, stepped):
    xd = _icm_frames().cuda()
    module = _icm_module(3)
    flat, nat = _icm_native(module)
    nat.encode(xd)
    if stepped:
        flat.grad.copy_(torch.randn_like(flat.grad) * 1e-2)
        flat.adam_step(1e-3, None)
        nat.encode(xd)
    old = _weights(module)
    target = _once("icm_new", lambda: {k: v.clone() for k, v in _icm_module(4).state_dict().items()})
    _write(route, module, flat, target)
    assert _same_sd(_weights(module), target)
    phi_old, phi_new = _phi64(old), _once("icm_phi_new", lambda: _phi64(target))
    assert (phi_new - phi_old).abs().max().item() >= 0.1 * phi_new.abs().max().item()

    def fresh():
        m = _icm_module(0)
        m.load_state_dict(target)
        _, n = _icm_native(m)
        return n.encode(xd)[1].clone()
    phi_fresh = _once("icm_fresh", fresh)
    phi = nat.encode(xd)[1].clone()
    torch.cuda.synchronize()
    assert torch.equal(phi.view(torch.int32), phi_fresh.view(torch.int32)), "phi bitwise a fresh NativeIcm's"
    # the bound of tests/test_icm_gpu.py::test_encode_vs_fp64
    scale = phi_new.abs().max().item()
    assert (phi.cpu().double() - phi_new).abs().max().item() <= 1e-5 * scale


# ---- product level: a checkpoint loaded into a running PPO
def _ppo(seed_np=0):
    import numpy as np
    import env as E
    import ppo
    np.random.seed(seed_np)
    torch.manual_seed(seed_np)  # (the policy's initial weights)
    env_id = "BreakoutNoFrameskip-v4"
    return ppo.PPO(env_id=env_id, env=E.DeviceAtariEnv(env_id, 8), n_envs=8, nstep=4, batch_size=32, n_epochs=1,
                   quiet=True, seed=3)


def _ckpt(alg, seed):
    import models
    n = alg.policy.action_dim
    torch.manual_seed(seed)
    return {k: v.clone() for k, v in models.CnnActorCritic(4, n).state_dict().items()}


def _act(alg, obs):
    torch.manual_seed(1)
    with torch.no_grad():
        logits = alg.policy.net(obs)[0].clone()
        a, v, lp = alg.policy.act(obs)
    torch.cuda.synchronize()
    return logits, v.clone(), lp.clone()


def test_ppo_acts_on_a_checkpoint_loaded_after_a_rollout():
    """one rollout (which packs the weights and captures the collect graph), load_state_dict of other weights into
    the policy, then act: bitwise a PPO that held those weights from the start"""
    g = torch.Generator(device="cuda").manual_seed(13)
    obs = torch.randint(0, 256, (8, 4, 84, 84), dtype=torch.uint8, device="cuda", generator=g)
    alg = _ppo()
    sd = _ckpt(alg, 77)
    alg.collect_samples()
    before = _act(alg, obs)[0]
    alg.policy.net.load_state_dict(sd)
    got = _act(alg, obs)
    ref = _ppo()
    ref.policy.net.load_state_dict(sd)  # before its first pass: nothing is packed yet
    ref.collect_samples()
    want = _act(ref, obs)
    assert not torch.equal(before, want[0]), "the checkpoint changes the logits"
    for name, a, b in zip(("logits", "values", "log-probs"), got, want):
        assert torch.equal(a, b), name


def test_ppo_collect_graph_replays_on_a_loaded_checkpoint():
    """the second rollout replays the captured collect graph on forms refreshed by pack(): after a load_state_dict it
    must be the rollout of a run that also called invalidate() by hand, the stronger form of the same refresh"""
    runs = []
    for by_hand in (False, True):
        alg = _ppo()
        sd = _ckpt(alg, 77)
        alg.collect_samples()
        first = alg.rollout.values.clone()
        alg.policy.net.load_state_dict(sd)
        if by_hand:
            alg.policy.net.conv_impl.invalidate()
        alg.collect_samples()
        torch.cuda.synchronize()
        ro = alg.rollout
        runs.append((first, ro.values.clone(), ro.actions.clone(), ro.log_probs.clone(), ro.obs_slots.clone()))
    for name, a, b in zip(("first values", "values", "actions", "log-probs", "frames"), *runs):
        assert torch.equal(a, b), name
