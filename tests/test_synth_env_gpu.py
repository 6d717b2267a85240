"""The synthetic device envs (csrc/env.hip) and their episode bookkeeping (csrc/episode.h) against
the numpy twins of tests/synth_env_twin.py (checked on the CPU by tests/test_synth_env_twin.py).
Everything compared is integers, float32 values k / 2^24 and sums of ones: the tolerance is zero
throughout.  Every buffer a kernel writes is a view into a sentinel-filled allocation
(tests/guarded.py), the floating-point ones pre-filled with NaN."""
import numpy as np
import pytest
import torch

import synth_env_twin as ST
from guarded import Arena
from oracle import philox as PH

pytestmark = pytest.mark.gpu

NAN = float("nan")
SEED = (0xC0FFEE << 32) | 0x51  # non-zero high key word
F32, I32, I64, U8 = torch.float32, torch.int32, torch.int64, torch.uint8


def _native():
    import native
    return native


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    return t.cpu().numpy()


def _same(t, ref):
    """exact, NaN positions included"""
    ref = np.asarray(ref)
    got = _np(t)
    return got.dtype == ref.dtype and got.shape == ref.shape and np.array_equal(
        got, ref, equal_nan=got.dtype.kind == "f")


class _Bufs:
    """The arrays one env step writes, each between guards."""

    def __init__(self, arena, n, obs_shape=None, obs_dtype=F32):
        self.rewards = arena.new(n, F32, init=NAN)
        self.dones = arena.new(n, U8)
        self.ep_ret = arena.new(n, F32, init=NAN)
        self.ep_len = arena.new(n, I32)
        self.done_ret = arena.new(n, F32, init=7.0)
        self.done_len = arena.new(n, I32)
        if obs_shape is not None:
            self.obs = arena.new(obs_shape, obs_dtype, init=NAN if obs_dtype == F32 else None)

    def episode(self):
        return dict(ep_ret=self.ep_ret, ep_len=self.ep_len, done_ret=self.done_ret, done_len=self.done_len)

    def matches(self, twin):
        return (_same(self.ep_ret, twin.ep_ret) and _same(self.ep_len, twin.ep_len)
                and _same(self.done_ret, twin.done_ret) and _same(self.done_len, twin.done_len))


def _actions(rs, n):
    return rs.randint(0, 3, n).astype(np.int32)


# ------------------------------------------------------------------ vector env, the kernel
VEC_CASES = [(1, 257), (3, 1), (4, 255), (5, 257), (11, 255), (24, 1), (24, 257), (3, 257)]


def _vec_run(D, N, discrete, p_done, max_len, steps=10, off=100):
    """reset + `steps` steps on guarded buffers against the twin; -> (number of dones, done_len values seen)"""
    native = _native()
    arena = Arena()
    b = _Bufs(arena, N, (N, D))
    twin = ST.SyntheticVec(N, D, SEED, p_done=p_done, max_len=max_len, env_offset=off, discrete=discrete)
    native.vec_env_reset(b.obs, N, D, off, SEED, b.ep_ret, b.ep_len)
    assert _same(b.obs, twin.reset())
    assert (b.ep_ret == 0).all() and (b.ep_len == 0).all()
    assert torch.isnan(b.rewards).all()  # the reset form writes neither rewards nor dones
    rs = np.random.RandomState(D * 1000 + N)
    n_done, lens = 0, set()
    for k in range(1, steps + 1):
        a = _actions(rs, N)
        b.obs.fill_(NAN)
        native.vec_env_step(b.obs, _dev(a) if discrete else None, N, D, off, SEED, k, p_done, max_len, b.rewards,
                            b.dones, **b.episode())
        obs, rew, done = twin.step(a)
        assert _same(b.obs, obs), k
        assert _same(b.rewards, rew) and _same(b.dones, done.astype(np.uint8)), k
        assert b.matches(twin), k
        n_done += int(done.sum())
        lens |= set(twin.done_len[done].tolist())
    arena.check()
    return n_done, lens


@pytest.mark.parametrize("discrete", [True, False], ids=["int32-actions", "actions-none"])
@pytest.mark.parametrize("D,N", VEC_CASES)
def test_vec_env_matches_twin(D, N, discrete):
    """Ten steps at p_done = 0.2, max_len = 4, env_offset = 100: observations (the `b*4 + j < D` tail at D % 4 != 0,
    the `n >= N` tail of the second block at N = 257), rewards, dones and the four episode arrays equal the twin at
    every step, with int32 actions and with actions = None (Box).  Guards round every array are intact."""
    n_done, lens = _vec_run(D, N, discrete, 0.2, 4)
    assert n_done >= 2
    if N > 1:
        assert lens == {1, 2, 3, 4}  # random ends and the time limit both happened


def test_vec_env_never_and_always_done():
    """max_len = 0 and p_done = 0: nothing ever ends; p_done = 1: every env ends every step, with done_len == 1."""
    assert _vec_run(5, 67, True, 0.0, 0, steps=12) == (0, set())
    assert _vec_run(5, 67, True, 1.0, 0, steps=3) == (3 * 67, {1})
    assert _vec_run(5, 67, True, 0.0, 1, steps=3) == (3 * 67, {1})
    assert _vec_run(3, 9, False, 0.0, 5, steps=11) == (2 * 9, {5})


def test_vec_env_without_episode_arrays():
    """ep_ret / ep_len null: the step still writes obs, rewards and dones; the time limit cannot apply."""
    native = _native()
    arena = Arena()
    N, D = 9, 6
    b = _Bufs(arena, N, (N, D))
    twin = ST.SyntheticVec(N, D, SEED, p_done=0.3, max_len=0, env_offset=2)
    native.vec_env_reset(b.obs, N, D, 2, SEED)
    assert _same(b.obs, twin.reset())
    for k in range(1, 4):
        a = _actions(np.random.RandomState(k), N)
        native.vec_env_step(b.obs, _dev(a), N, D, 2, SEED, k, 0.3, 2, b.rewards, b.dones)
        obs, rew, done = twin.step(a)
        assert _same(b.obs, obs) and _same(b.dones, done.astype(np.uint8)) and (b.rewards == 1).all()
    assert torch.isnan(b.ep_ret).all() and (b.done_ret == 7).all()
    arena.check()


def test_vec_env_shard_equals_rows_of_the_full_run():
    """env_offset = 4, N = 4 == rows 4..7 of the run of envs [0, 8): observations, dones, episode arrays."""
    native = _native()
    arena = Arena()
    D, steps = 5, 8
    full, part = _Bufs(arena, 8, (8, D)), _Bufs(arena, 4, (4, D))
    native.vec_env_reset(full.obs, 8, D, 0, SEED, full.ep_ret, full.ep_len)
    native.vec_env_reset(part.obs, 4, D, 4, SEED, part.ep_ret, part.ep_len)
    assert torch.equal(part.obs, full.obs[4:])
    rs = np.random.RandomState(3)
    ended = 0
    for k in range(1, steps + 1):
        a = _dev(_actions(rs, 8))
        native.vec_env_step(full.obs, a, 8, D, 0, SEED, k, 0.2, 4, full.rewards, full.dones, **full.episode())
        native.vec_env_step(part.obs, a[4:].contiguous(), 4, D, 4, SEED, k, 0.2, 4, part.rewards, part.dones,
                            **part.episode())
        for name in ("obs", "rewards", "dones", "ep_ret", "ep_len", "done_len"):
            assert torch.equal(getattr(part, name), getattr(full, name)[4:]), (k, name)
        assert _same(part.done_ret, _np(full.done_ret)[4:]), k
        ended += int(part.dones.sum())
    assert ended >= 4
    arena.check()


def test_vec_env_reset_zeroes_the_running_episode():
    native = _native()
    arena = Arena()
    N, D = 5, 3
    b = _Bufs(arena, N, (N, D))
    native.vec_env_reset(b.obs, N, D, 0, SEED, b.ep_ret, b.ep_len)
    first = b.obs.clone()
    for k in (1, 2):
        native.vec_env_step(b.obs, None, N, D, 0, SEED, k, 0.0, 0, b.rewards, b.dones, **b.episode())
    assert (b.ep_ret == 2).all() and (b.ep_len == 2).all() and not torch.equal(b.obs, first)
    native.vec_env_reset(b.obs, N, D, 0, SEED, b.ep_ret, b.ep_len)
    assert (b.ep_ret == 0).all() and (b.ep_len == 0).all() and torch.equal(b.obs, first)
    arena.check()


def test_vec_env_refusals():
    """step must lie in [1, 2^32): step 0 is the reset draw, 2^32 would wrap onto it."""
    native = _native()
    arena = Arena()
    N, D = 4, 3
    b = _Bufs(arena, N, (N, D))
    for step in (0, 2 ** 32, -1):
        with pytest.raises(native.NativeError, match="step must be in"):
            native.vec_env_step(b.obs, None, N, D, 0, SEED, step, 0.1, 0, b.rewards, b.dones, **b.episode())
    for kw in (dict(N=0), dict(D=0)):
        args = dict(N=N, D=D)
        args.update(kw)
        with pytest.raises(native.NativeError, match="bad arguments"):
            native.vec_env_step(b.obs, None, args["N"], args["D"], 0, SEED, 1, 0.1, 0, b.rewards, b.dones)
        with pytest.raises(native.NativeError, match="bad arguments"):
            native.vec_env_reset(b.obs, args["N"], args["D"], 0, SEED)
    with pytest.raises(native.NativeError, match="bad arguments"):
        native.vec_env_step(b.obs, None, N, D, 0, SEED, 1, 0.1, 0, None, b.dones)
    assert torch.isnan(b.obs).all() and torch.isnan(b.rewards).all() and torch.isnan(b.ep_ret).all()
    native.vec_env_step(b.obs, None, N, D, 0, SEED, 2 ** 32 - 1, 0.1, 0, b.rewards, b.dones)  # the last step
    twin = ST.SyntheticVec(N, D, SEED, discrete=False)
    twin.k = 2 ** 32 - 2
    assert _same(b.obs, twin.step()[0])
    arena.check()


# ------------------------------------------------------------------ vector env, the class
@pytest.mark.parametrize("env_id,D,discrete", [("Hopper-v2", 11, False), ("CartPole-v1", 4, True)])
def test_device_vec_env_class(env_id, D, discrete):
    """DeviceVecEnv.reset() / step(): the twin's stream (Box actions dropped, Discrete ones in the counter), and
    episode_infos reports exactly the finished episodes with their return and length."""
    import env as E
    N, off = 6, 10
    dev = E.DeviceVecEnv(env_id, N, seed=SEED, env_offset=off, p_done=0.2, max_len=4)
    assert dev.obs_dim == D and (dev.action_space.__class__.__name__ == "Discrete") == discrete
    twin = ST.SyntheticVec(N, D, SEED, p_done=0.2, max_len=4, env_offset=off, discrete=discrete)
    assert _same(dev.reset(), twin.reset())
    rs = np.random.RandomState(5)
    finished = 0
    for k in range(1, 11):
        a = rs.randint(0, 2, N) if discrete else rs.randn(N, 3).astype(np.float32)
        obs, rew, done, infos = dev.step(a)
        t_obs, t_rew, t_done = twin.step(a if discrete else None)
        assert _same(obs, t_obs) and _same(rew, t_rew) and _same(done, t_done), k
        assert infos == ST.episode_infos(twin.done_ret, twin.done_len), k
        assert [bool(i) for i in infos] == list(t_done)
        assert _same(dev.ep_ret, twin.ep_ret) and _same(dev.ep_len, twin.ep_len), k
        finished += len([i for i in infos if i])
    assert finished >= 6 and dev.k == 10


# ------------------------------------------------------------------ Atari env
def test_atari_env_episode_arrays_match_twin():
    """N = 5, 12 steps, p_done = 0.3, p_reward = 0.4: ep_ret, ep_len, done_ret (NaN positions included) and done_len
    equal the twin with the bookkeeping round it; a finished env has three zeroed frames and the new one last."""
    native = _native()
    arena = Arena()
    N, off = 5, 7
    b = _Bufs(arena, N)
    twin = ST.AtariEpisodes(N, SEED, p_reward=0.4, p_done=0.3, env_offset=off)
    obs = arena.new((N, 4, 84, 84), U8)
    nxt = arena.new((N, 4, 84, 84), U8)
    native.atari_env_reset(obs, N, off, SEED, b.ep_ret, b.ep_len)
    assert _same(obs, twin.reset()) and (b.ep_ret == 0).all() and (b.ep_len == 0).all()
    rs = np.random.RandomState(2)
    ended, paid = 0, 0.0
    for k in range(1, 13):
        a = rs.randint(0, 4, N).astype(np.int32)
        native.atari_env_step(obs, nxt, _dev(a), N, off, SEED, k, 0.4, 0.3, b.rewards, b.dones, **b.episode())
        t_obs, t_rew, t_done, _ = twin.step(a)
        assert _same(b.rewards, t_rew) and _same(b.dones, t_done.astype(np.uint8)), k
        assert b.matches(twin), k
        if k == 12 or (t_done.any() and not ended):
            assert _same(nxt, t_obs), k
        ended += int(t_done.sum())
        paid += float(np.nansum(twin.done_ret))
        obs, nxt = nxt, obs
    assert ended >= 5 and paid >= 2  # episodes ended, some with a return
    arena.check()


@pytest.mark.parametrize("off", [1, 16])
@pytest.mark.parametrize("base", [0, 1000, 2 ** 31 + 5])
def test_atari_env_step_dc_reads_the_device_counter(base, off):
    """atari_env_step_dc(step_base = [base], step_off = off) writes the stacks, rewards, dones and episode arrays
    of atari_env_step(step = base + off): the form the captured collect graph replays."""
    native = _native()
    arena = Arena()
    N = 3
    start = arena.new((N, 4, 84, 84), U8)
    native.atari_env_reset(start, N, 0, SEED)
    a = _dev(np.array([1, 0, 3], np.int32))
    outs = []
    for dc in (False, True):
        b = _Bufs(arena, N, (N, 4, 84, 84), U8)
        b.ep_ret.fill_(2.0)
        b.ep_len.fill_(5)
        if dc:
            counter = arena.new(1, I64, init=base)
            native.atari_env_step_dc(start, b.obs, a, N, 0, SEED, counter, off, 0.5, 0.5, b.rewards, b.dones,
                                     **b.episode())
            assert int(counter) == base
        else:
            native.atari_env_step(start, b.obs, a, N, 0, SEED, base + off, 0.5, 0.5, b.rewards, b.dones,
                                  **b.episode())
        outs.append(b)
    for name in ("obs", "rewards", "dones", "ep_ret", "ep_len", "done_len"):
        assert torch.equal(getattr(outs[0], name), getattr(outs[1], name)), name
    assert _same(outs[1].done_ret, _np(outs[0].done_ret))
    frame = PH.atari_frame(SEED, np.arange(N), base + off, [1, 0, 3]).reshape(N, 84, 84)
    assert np.array_equal(_np(outs[1].obs[:, 3]), frame)
    arena.check()


def test_atari_env_step_dc_refuses_a_null_counter():
    native = _native()
    arena = Arena()
    N = 2
    b = _Bufs(arena, N, (N, 4, 84, 84), U8)
    start = torch.zeros((N, 4, 84, 84), dtype=U8, device="cuda")
    a = torch.zeros(N, dtype=I32, device="cuda")
    with pytest.raises(native.NativeError, match="null step counter"):
        native.atari_env_step_dc(start, b.obs, a, N, 0, SEED, None, 1, 0.5, 0.5, b.rewards, b.dones, **b.episode())
    for step in (0, 2 ** 32):
        with pytest.raises(native.NativeError, match="step must be in"):
            native.atari_env_step(start, b.obs, a, N, 0, SEED, step, 0.5, 0.5, b.rewards, b.dones, **b.episode())
    assert torch.isnan(b.rewards).all() and torch.isnan(b.ep_ret).all()
    arena.check()


# ------------------------------------------------------------------ counters
@pytest.mark.parametrize("delta", [1, -3, 2 ** 40])
@pytest.mark.parametrize("n", [1, 2, 64])
def test_counters_add(n, delta):
    """The first n of 64 int64 counters gain delta (the collect graph's step / sample counters); the others and the
    guards stay."""
    native = _native()
    arena = Arena()
    before = np.arange(64, dtype=np.int64) * 1_000_003 - 17
    buf = arena.new(64, I64, init=before)
    native.counters_add(buf[:n], delta)
    native.counters_add(buf[:n], delta)
    expect = before.copy()
    expect[:n] += 2 * delta
    assert _same(buf, expect)
    arena.check()


def test_counters_add_refusals():
    native = _native()
    arena = Arena()
    buf = arena.new(65, I64, init=5)
    for bad in (buf[:0], buf):
        with pytest.raises(native.NativeError, match="ppox_counters_add"):
            native.counters_add(bad, 1)
    assert (buf == 5).all()
    arena.check()
