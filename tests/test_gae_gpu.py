"""K1 GAE on the GPU through the C ABI vs the golden fixtures and the oracle.
Bit-exact (np.array_equal) at every size."""
import numpy as np
import pytest
import torch

from oracle import gae as G

pytestmark = pytest.mark.gpu


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.cuda()


def _run_single(rew, val, done, lv, ld, gamma, lam):
    import native
    T, N = rew.shape
    adv = torch.empty(T, N, device="cuda")
    ret = torch.empty(T, N, device="cuda")
    native.gae(_dev(rew), _dev(val), _dev(done, torch.uint8), _dev(lv), _dev(ld, torch.uint8),
               gamma, lam, adv, ret)
    torch.cuda.synchronize()
    return adv.cpu().numpy(), ret.cpu().numpy()


def test_gae_golden(golden):
    f = golden("gae_single")
    for k in range(int(f["ncases"])):
        p = f"c{k}_"
        adv, ret = _run_single(f[p + "rewards"], f[p + "values"], f[p + "dones"], f[p + "last_value"],
                               f[p + "last_done"], float(f[p + "gamma"]), float(f[p + "lam"]))
        assert np.array_equal(adv, f[p + "advantages"]), p
        assert np.array_equal(ret, f[p + "returns"]), p


def test_gae_dual_golden(golden):
    import native
    f = golden("gae_dual")
    for k in range(int(f["ncases"])):
        p = f"c{k}_"
        T, N = f[p + "rewards"].shape
        outs = [torch.empty(T, N, device="cuda") for _ in range(4)]
        native.gae_dual(_dev(f[p + "rewards"]), _dev(f[p + "values"]), _dev(f[p + "dones"], torch.uint8),
                        _dev(f[p + "last_value"]), _dev(f[p + "last_done"], torch.uint8),
                        _dev(f[p + "int_rewards"]), _dev(f[p + "int_values"]), _dev(f[p + "last_int_value"]),
                        float(f[p + "gamma"]), float(f[p + "int_gamma"]), float(f[p + "lam"]), *outs)
        torch.cuda.synchronize()
        for o, key in zip(outs, ("advantages", "returns", "int_advantages", "int_returns")):
            assert np.array_equal(o.cpu().numpy(), f[p + key]), (p, key)


@pytest.mark.parametrize("T,N", [(128, 4096), (128, 131072 + 4), (128, 131072), (3, 5), (1, 200000), (16, 262144),
                                 (8, 262144 + 2), (4, 131071)])
def test_gae_random_vs_oracle(T, N):
    """Covers every lane width (1 env/lane, float2 lanes from N = 131,072, float4 lanes from
    262,144; odd N falls back to 1 env/lane) and ragged N."""
    rs = np.random.RandomState(T * 7 + N)
    rew = (rs.rand(T, N) < 0.02).astype(np.float32) + rs.randn(T, N).astype(np.float32) * 0.1
    val = rs.randn(T, N).astype(np.float32)
    done = rs.rand(T, N) < 0.01
    lv = rs.randn(N).astype(np.float32)
    ld = done[-1]
    adv, ret = _run_single(rew, val, done, lv, ld, 0.99, 0.95)
    eadv, eret = G.gae_single(rew, val, done, lv, ld, 0.99, 0.95)
    assert np.array_equal(adv, eadv)
    assert np.array_equal(ret, eret)


def test_gae_dual_random_vs_oracle():
    import native
    T, N = 128, 131072
    rs = np.random.RandomState(5)
    a = [rs.randn(T, N).astype(np.float32) for _ in range(4)]
    done = rs.rand(T, N) < 0.01
    lv, liv = rs.randn(N).astype(np.float32), rs.randn(N).astype(np.float32)
    outs = [torch.empty(T, N, device="cuda") for _ in range(4)]
    native.gae_dual(_dev(a[0]), _dev(a[1]), _dev(done, torch.uint8), _dev(lv), _dev(done[-1], torch.uint8),
                    _dev(a[2]), _dev(a[3]), _dev(liv), 0.99, 0.999, 0.95, *outs)
    torch.cuda.synchronize()
    exp = G.gae_dual(a[0], a[2], a[1], a[3], done, lv, liv, done[-1], 0.99, 0.999, 0.95)
    for o, e in zip(outs, exp):
        assert np.array_equal(o.cpu().numpy(), e)


# ----------------------------------------------------------------- every dispatch branch, tail and alignment
# launch_gae picks one of three forms by size and alignment (csrc/gae.hip): the staged form while N <= 8192,
# T <= 256 and the (T, envs-per-block) tile fits 64 KB of LDS (one stream: T <= 170 at 16 envs; two: T <= 227
# at 8), else lanes of 4 / 2 / 1 envs (float4 from N = 262,144, float2 from 131,072, given N % lanes == 0 and
# every base pointer aligned to the lane).  Outputs are carved out of sentinel-filled buffers (tests/guarded.py).
def _data(T, N, seed, density=0.01, scale=1.0):
    """last_done is drawn independently of done[-1] (the rollout's last flag is not the step's)."""
    rs = np.random.RandomState(seed)
    d = {k: (rs.randn(T, N) * scale).astype(np.float32) for k in ("rew", "val", "irew", "ival")}
    d["done"] = rs.rand(T, N) < density
    d["ld"] = rs.rand(N) < 0.3
    d["lv"] = (rs.randn(N) * scale).astype(np.float32)
    d["liv"] = (rs.randn(N) * scale).astype(np.float32)
    return d


def _oracle(d, dual, gamma, lam, int_gamma):
    out = list(G.gae_single(d["rew"], d["val"], d["done"], d["lv"], d["ld"], gamma, lam))
    if dual:
        out += list(G.gae_intrinsic(d["irew"], d["ival"], d["liv"], int_gamma, lam))
    return out


def _run(d, dual, gamma=0.99, lam=0.95, int_gamma=0.999, off=None):
    """The kernel on `d` with every tensor carved from a guarded buffer; off: byte offsets from a 16-byte
    boundary by tensor name ('out' = every output)."""
    import native
    from guarded import Arena
    off = off or {}
    ar = Arena()
    T, N = d["rew"].shape
    f32, u8 = torch.float32, torch.uint8
    t = {k: ar.new(d[k].shape, u8 if d[k].dtype == bool else f32, off.get(k, 0), init=d[k].astype(np.uint8)
                   if d[k].dtype == bool else d[k]) for k in d}
    outs = [ar.new((T, N), f32, off.get("out", 0)) for _ in range(4 if dual else 2)]
    if dual:
        native.gae_dual(t["rew"], t["val"], t["done"], t["lv"], t["ld"], t["irew"], t["ival"], t["liv"], gamma,
                        int_gamma, lam, *outs)
    else:
        native.gae(t["rew"], t["val"], t["done"], t["lv"], t["ld"], gamma, lam, *outs)
    ar.check()
    for k in d:  # the inputs are read-only
        assert np.array_equal(t[k].cpu().numpy().astype(d[k].dtype), d[k]), k
    return [o.cpu().numpy() for o in outs]


def _same(got, exp, what):
    names = ("advantages", "returns", "int_advantages", "int_returns")
    for g, e, name in zip(got, exp, names):
        assert g.dtype == e.dtype == np.float32
        assert np.array_equal(g.view(np.uint32), e.view(np.uint32)), (what, name)


ONE_STREAM = [(1, 1), (1, 17), (16, 16), (33, 31), (170, 16), (171, 16), (256, 3), (257, 3), (17, 8192), (17, 8193)]
TWO_STREAMS = [(1, 9), (3, 5), (33, 4099), (227, 8), (228, 8), (17, 8193), (4, 131072), (4, 131073), (4, 262144),
               (4, 262146)]


@pytest.mark.parametrize("T,N", ONE_STREAM)
def test_gae_one_stream_branches(T, N):
    """The LDS limit (T = 170 / 171 at 16 envs per block), STAGED_TMAX (256 / 257), STAGED_NMAX (8192 / 8193),
    T off the 16-step chain chunk, one env, one step."""
    d = _data(T, N, 11 * T + N, density=0.05)
    _same(_run(d, False), _oracle(d, False, 0.99, 0.95, 0.0), (T, N))


@pytest.mark.parametrize("T,N", TWO_STREAMS)
def test_gae_two_stream_branches(T, N):
    """Two streams: staged with ragged N and at its LDS limit (T = 227 / 228 at 8 envs per block), one env per
    lane in 64- and (odd N >= 65,536) 256-thread blocks, float2 lanes, float4 lanes and float2 again at
    N = 262,146."""
    d = _data(T, N, 13 * T + N, density=0.05)
    _same(_run(d, True), _oracle(d, True, 0.99, 0.95, 0.999), (T, N))


@pytest.fixture(scope="module")
def aligned_case():
    d = _data(4, 262144, 77, density=0.05)
    return d, {dual: _oracle(d, dual, 0.99, 0.95, 0.999) for dual in (False, True)}, {}


@pytest.mark.parametrize("dual", [False, True])
@pytest.mark.parametrize("off", [{"rew": 4}, {"out": 8}, {"done": 1}, {"done": 2}, {"ld": 1}], ids=str)
def test_gae_alignment_fallbacks(aligned_case, off, dual):
    """fits(): a base pointer off its 16 bytes sends float4-sized work to float2 lanes (8 bytes off; dones 2 off)
    or to one env per lane (4 bytes off; dones / last_done 1 off).  Same bits as the aligned run and the oracle."""
    d, exp, aligned = aligned_case
    if dual not in aligned:
        aligned[dual] = _run(d, dual)
        _same(aligned[dual], exp[dual], "aligned")
    got = _run(d, dual, off=off)
    _same(got, aligned[dual], off)
    _same(got, exp[dual], off)


@pytest.mark.parametrize("density", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("T,N", [(33, 31), (17, 8193), (4, 262144)], ids=["staged", "lane", "float4"])
def test_gae_data_edges(T, N, density):
    """No episode end, every other step one, all of them; last_done drawn apart from done[-1]; gamma and lambda
    at 1 and 0; both intrinsic discounts; values of 1e6, where the f64 -> f32 casts of the carry round."""
    d = _data(T, N, int(7 * T + N + 10 * density), density=density, scale=1e6)
    for gamma, lam in [(1.0, 1.0), (0.999, 0.0), (0.0, 0.95)]:
        _same(_run(d, False, gamma, lam), _oracle(d, False, gamma, lam, 0.0), (gamma, lam))
        for int_gamma in (0.999, 0.99):
            _same(_run(d, True, gamma, lam, int_gamma), _oracle(d, True, gamma, lam, int_gamma),
                  (gamma, lam, int_gamma))
