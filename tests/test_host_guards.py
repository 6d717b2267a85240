"""Host-side guards that need no GPU."""
import pytest
import torch

import icm as icm_native


def _bare_icm():
    nat = object.__new__(icm_native.NativeIcm)
    nat._bufs, nat._captured = {}, set()

    class _Flat:
        device = torch.device("cpu")
    nat.flat = _Flat()
    return nat


def test_captured_icm_workspace_cannot_grow(monkeypatch):
    """A workspace the collect graph captured (icm.py _buf) raises instead of being
    silently replaced by a larger allocation the replayed graph would not see."""
    nat = _bare_icm()
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    a = nat._buf("ir", (8,))
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    assert nat._buf("ir", (8,)).data_ptr() == a.data_ptr()  # captured at this size
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    assert nat._buf("ir", (4,)).data_ptr() == a.data_ptr()  # smaller views are fine
    with pytest.raises(RuntimeError, match="captured"):
        nat._buf("ir", (16,))
    with pytest.raises(RuntimeError, match="captured"):
        nat._buf("ir", (8,), torch.int32)
    b = nat._buf("mb_phi", (4,))  # uncaptured tags still grow
    assert nat._buf("mb_phi", (64,)).numel() == 64 and b.numel() == 4


def _bare_comm(inflight=False, handle=1):
    import native
    c = object.__new__(native.DpComm)
    c.handle, c.world, c.rank, c.inflight = handle, 2, 0, inflight
    return c


def test_dp_comm_refuses_a_second_async_reduction():
    """one asynchronous reduction in flight at a time on the native communicator (a second
    one before the join is refused — csrc/dp.cpp returns the same error); a closed communicator refuses all."""
    import native
    t = torch.zeros(4)
    with pytest.raises(native.NativeError, match="in flight"):
        _bare_comm(inflight=True).all_reduce_(t, wait=False)
    with pytest.raises(native.NativeError, match="closed"):
        _bare_comm(handle=None).all_reduce_(t)
    assert _bare_comm(handle=None).close() == 0  # idempotent


def test_dist_shutdown_closes_the_native_communicator(monkeypatch):
    """dist.shutdown() destroys the process's native communicator (before the process group goes) and forgets
    it; a second call is a no-op."""
    import dist
    closed = []

    class _Comm:
        def close(self):
            closed.append(1)
            return 0
    monkeypatch.setattr(dist, "_dp_comm", _Comm())
    assert dist.shutdown() == 0 and closed == [1] and dist._dp_comm is None
    assert dist.shutdown() is None and closed == [1]


# ---- the packed weight forms' keys follow every write to the weights that the host can see (INTEGRATION.md:
# writes through torch move a version counter, any other write is announced by FlatParams.touch())
def _cpu_trunk():
    """a CnnActorCritic re-homed into one CPU flat buffer with its trunk and Adam-amax link attached (no kernel
    runs: only the keys are read)"""
    import convs
    import models
    torch.manual_seed(4)
    net = models.CnnActorCritic(4, 6)
    flat = models.FlatParams(net, "cpu")
    cv = convs.attach(net, flat, "split")
    assert cv._wmax is not None and flat.wmax is cv._wmax
    return net, flat, cv


def _keys(flat, cv):
    return cv.weights_key(), cv._wmax._key(flat)


def _write(route, net, flat):
    if route == "load_state_dict":
        net.load_state_dict({k: v.clone() for k, v in net.state_dict().items()})
    elif route == "param_copy":
        with torch.no_grad():
            for p in net.parameters():
                p.copy_(p * 2)
    elif route == "flat_copy":
        flat.data[:flat.n].copy_(flat.data[:flat.n] * 2)
    elif route == "data_copy":
        for p in net.parameters():
            p.data.copy_(p.data * 2)
    elif route == "raw_buffer":  # a write outside torch, as a native kernel's or a collective's
        flat.data.numpy()[:flat.n] *= 2
    elif route == "touch":
        flat.touch()
    else:
        raise ValueError(route)


@pytest.mark.parametrize("route", ["load_state_dict", "param_copy", "flat_copy", "touch"])
def test_weight_write_moves_the_pack_and_fold_keys(route):
    net, flat, cv = _cpu_trunk()
    pack0, fold0 = _keys(flat, cv)
    _write(route, net, flat)
    pack1, fold1 = _keys(flat, cv)
    assert pack1 != pack0, "NatureConvs.pack would keep the forms of the old weights"
    assert fold1 != fold0, "WmaxLink would split the new weights at the old step's exponent"


@pytest.mark.parametrize("route", ["data_copy", "raw_buffer"])
def test_counterless_write_needs_touch(route):
    """x.data.copy_() and a write on the raw buffer move no torch counter and so no key: why touch() exists"""
    net, flat, cv = _cpu_trunk()
    w0 = flat.data.clone()
    keys0 = _keys(flat, cv)
    _write(route, net, flat)
    assert not torch.equal(flat.data, w0), "the weights did change"
    assert _keys(flat, cv) == keys0
    flat.touch()
    pack1, fold1 = _keys(flat, cv)
    assert pack1 != keys0[0] and fold1 != keys0[1]


@pytest.mark.parametrize("route", ["load_state_dict", "flat_copy", "touch"])
def test_icm_pack_key_follows_writes(route):
    import models
    from env import Discrete
    from util import ActionConverter
    torch.manual_seed(2)
    m = models.IntrinsicCuriosityModule(128, ActionConverter(Discrete(4)), 32)
    flat = models.FlatParams(m, "cpu")
    w1 = m.state_encoder[0].weight
    k0 = flat.write_key((w1,))
    _write(route, m, flat)
    assert flat.write_key((w1,)) != k0
    k1 = flat.write_key((w1,))
    w1.data.copy_(w1.data * 2)
    assert flat.write_key((w1,)) == k1


def test_bias_only_write_repacks_but_keeps_the_fold():
    """the forms' tails hold bias bounds, so a conv bias written alone moves the pack key; the Adam step's amax
    partials cover the five weight tensors only and stay valid"""
    net, flat, cv = _cpu_trunk()
    pack0, fold0 = _keys(flat, cv)
    with torch.no_grad():
        net.feature_extractor[2].bias.add_(1.0)
    pack1, fold1 = _keys(flat, cv)
    assert pack1 != pack0 and fold1 == fold0


def test_fold_bookkeeping_survives_the_new_key():
    """recorded() at the step, for_pack() with nothing written between: the packing reads the step's partials;
    any write between (counter or touch()) sends it back to its own amax pass"""
    net, flat, cv = _cpu_trunk()
    lk = cv._wmax
    flat.step_count += 1  # FlatParams.adam_step's bookkeeping without its kernel
    assert lk.ready(flat)
    rec = lk.recording()
    lk.recorded(flat)
    assert lk.valid is not None and lk.valid[0][0] == flat.step_count
    amax_in, amax_next = lk.for_pack(flat)
    assert amax_in is not None and amax_in.data_ptr() == rec.data_ptr() and amax_next.data_ptr() != rec.data_ptr()
    assert lk.folds == 1
    for route in ("load_state_dict", "param_copy", "flat_copy", "touch"):
        flat.step_count += 1
        assert lk.ready(flat)
        lk.recorded(flat)
        _write(route, net, flat)
        amax_in, _ = lk.for_pack(flat)
        assert amax_in is None and lk.valid is None and lk.folds == 1, route


def test_pack_hit_path_compares_the_full_key_once_per_pass(monkeypatch):
    """pack()'s early return: a pass's first call (forward_acts) compares the whole key, the calls inside the pass
    (in_pass) the step count and touch() generation alone — and fall through to the whole key when those moved"""
    net, flat, cv = _cpu_trunk()
    B = 37
    key = cv._pack_key(B)
    cv._version, cv._last_batch = cv.weights_key(), key  # as after a packing at B rows
    cv._quick = (flat.step_count, flat.gen)
    cv._packed = set(cv._forms(B))
    calls = []
    real = flat.write_key
    monkeypatch.setattr(flat, "write_key", lambda t=(): calls.append(1) or real(t))
    assert cv.pack(B) is False and len(calls) == 1
    assert cv.pack(B, in_pass=True) is False and len(calls) == 1
    flat.touch()
    cv._forms = lambda batch: set()  # (no kernel on the CPU: nothing to pack)
    cv._forms_cache.clear()
    assert cv.pack(B, in_pass=True) is False and len(calls) == 2, "a touch() reaches the calls inside a pass too"
    assert cv._version == cv.weights_key() and cv._packed == set()
