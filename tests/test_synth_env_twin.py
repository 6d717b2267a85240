"""CPU checks of tests/synth_env_twin.py: the episode bookkeeping against a trace written out by
hand, and the Atari twin with the bookkeeping round it against oracle.philox.SyntheticAtari."""
import numpy as np

import synth_env_twin as ST
from oracle import philox as PH

NAN = np.nan


def test_episode_mixin_hand_trace():
    """Two envs, six steps.  Env 0 earns 1, 0, 1 and ends at step 3, then 0, 1 and ends at step 5, then 1;
    env 1 earns 0.5 every step and ends at steps 1 and 6."""
    ep = ST.Episode()
    ep.ep_reset(2)
    assert ep.ep_ret.dtype == np.float32 and ep.ep_len.dtype == np.int32
    assert np.isnan(ep.done_ret).all() and (ep.done_len == 0).all()
    rew = [(1, .5), (0, .5), (1, .5), (0, .5), (1, .5), (1, .5)]
    done = [(0, 1), (0, 0), (1, 0), (0, 0), (1, 0), (0, 1)]
    ep_ret = [(1, 0), (1, .5), (0, 1), (0, 1.5), (0, 2), (1, 0)]
    ep_len = [(1, 0), (2, 1), (0, 2), (1, 3), (0, 4), (1, 0)]
    done_ret = [(NAN, .5), (NAN, NAN), (2, NAN), (NAN, NAN), (1, NAN), (NAN, 2.5)]
    done_len = [(0, 1), (0, 0), (3, 0), (0, 0), (2, 0), (0, 5)]
    for t in range(6):
        ep.ep_update(np.array(rew[t], np.float32), np.array(done[t], bool))
        assert np.array_equal(ep.ep_ret, np.array(ep_ret[t], np.float32)), t
        assert np.array_equal(ep.ep_len, np.array(ep_len[t], np.int32)), t
        assert np.array_equal(ep.done_ret, np.array(done_ret[t], np.float32), equal_nan=True), t
        assert np.array_equal(ep.done_len, np.array(done_len[t], np.int32)), t
        assert ep.done_ret.dtype == np.float32 and ep.done_len.dtype == np.int32


def test_atari_with_episodes_returns_what_the_oracle_twin_returns():
    """Same frames, rewards and dones as SyntheticAtari; the episode arrays are the running sums of them."""
    n, seed, off = 5, (7 << 32) | 11, 3
    plain = PH.SyntheticAtari(n, seed, p_reward=0.4, p_done=0.3, env_offset=off)
    wrapped = ST.AtariEpisodes(n, seed, p_reward=0.4, p_done=0.3, env_offset=off)
    assert np.array_equal(plain.reset(), wrapped.reset())
    rs = np.random.RandomState(0)
    ret, ln, ended = np.zeros(n), np.zeros(n, int), 0
    for k in range(1, 13):
        a = rs.randint(0, 4, n)
        o1, r1, d1, _ = plain.step(a)
        o2, r2, d2, _ = wrapped.step(a)
        assert np.array_equal(o1, o2) and np.array_equal(r1, r2) and np.array_equal(d1, d2), k
        ret, ln = ret + r1, ln + 1
        assert np.array_equal(wrapped.done_ret, np.where(d1, ret, NAN).astype(np.float32), equal_nan=True), k
        assert np.array_equal(wrapped.done_len, np.where(d1, ln, 0)), k
        ret[d1], ln[d1] = 0, 0
        assert np.array_equal(wrapped.ep_ret, ret.astype(np.float32)) and np.array_equal(wrapped.ep_len, ln), k
        ended += int(d1.sum())
    assert ended >= 5  # the run ends episodes, some with a non-zero return
    infos = ST.episode_infos(wrapped.done_ret, wrapped.done_len)
    assert [bool(i) for i in infos] == list(d1)


def test_as_u32_is_the_kernels_cast():
    assert list(ST.as_u32(np.array([0, 3, -1, 2 ** 31 - 1], np.int32), 4)) == [0, 3, 0xFFFFFFFF, 2 ** 31 - 1]
