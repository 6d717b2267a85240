"""tests/sil_twin.py (the definition of PPO(sil=True)) against the reference's running
parts recorded in tests/golden/sil.npz (tests/golden/make_golden_sil.py).  CPU only."""
import numpy as np
import pytest

import sil_twin as T


@pytest.fixture
def sil(golden):
    return golden("sil")


@pytest.mark.parametrize("name", ["t64", "t8", "buf"])
def test_rebuild_is_bitwise_the_reference_tree(sil, name):
    """Bottom-up from the reference's own leaves = the tree its leaf-by-leaf writes reached."""
    ref_s, ref_m = sil[name + "_sum"], sil[name + "_min"]
    P = len(ref_s) // 2
    s, m = T.rebuild(ref_s[P:], ref_m[P:])
    assert np.array_equal(s[1:], ref_s[1:]) and np.array_equal(m[1:], ref_m[1:])  # (node 0 is unused)


def test_set_leaf_replays_the_write_sequence(sil):
    for name, P in (("t64", 64), ("t8", 8)):
        s, m = np.zeros(2 * P), np.full(2 * P, np.inf)
        for i, x in zip(sil[name + "_widx"], sil[name + "_wval"]):
            T.set_leaf(s, int(i), float(x), lambda a, b: a + b)
            T.set_leaf(m, int(i), float(x) if x > 0 else np.inf, min)
        assert np.array_equal(s[1:], sil[name + "_sum"][1:]) and np.array_equal(m[1:], sil[name + "_min"][1:])


def test_prefixsum_guard_is_never_weaker_than_the_reference(sil):
    """Every leaf positive: the guarded descent is find_prefixsum_idx, for 20,000 uniforms, u = 0 and
    u = 1 - 2^-53."""
    u = sil["pos_u"]
    assert u[-2] == 0.0 and u[-1] == 1.0 - 2.0 ** -53 and len(u) == 20002
    assert (sil["pos_sum"][64:] > 0).all()
    assert np.array_equal(T.sample_indices(sil["pos_sum"], u), sil["pos_idx"])


def test_guard_skips_an_empty_right_child():
    """left <= mass and right == 0: the reference's descent would end on the empty leaf."""
    s, _ = T.rebuild(np.array([0.25, 0.5, 0.0, 0.0]), np.full(4, np.inf))
    assert T.find_prefixsum_idx(s, 0.75) == 1       # mass == root: left 0.75 <= mass, right 0
    assert T.find_prefixsum_idx(s, 0.25) == 1
    assert T.find_prefixsum_idx(s, 0.0) == 0


@pytest.mark.parametrize("beta", [0.0, 0.4, 1.0])
def test_weights_match_the_reference(sil, beta):
    tag = f"buf_b{beta:g}_"
    idx = sil[tag + "idx"]
    n = int(sil["buf_cfg"][1])  # len(buffer)
    w = T.weights(sil["buf_sum"], sil["buf_min"], n, idx, beta)
    if beta == 0.0:
        # the reference leaves self.weights untouched at beta 0 (buffer.py:464); the limit of w / max_w is 1
        assert sil[tag + "weights"].size == 0 and np.array_equal(w, np.ones(len(idx)))
        return
    ref = sil[tag + "weights"]
    assert len(ref) == len(idx) == 16
    assert np.max(np.abs(w - ref) / np.abs(ref)) <= 1e-15


class _Trees:
    pass


def test_update_priorities_last_occurrence_wins(sil):
    """The reference's update (buffer.py:454-459) with repeated indices, from its own tree state."""
    t = _Trees()
    t.sum_tree, t.min_tree = sil["buf_sum"].copy(), sil["buf_min"].copy()
    t.max_priority, t.alpha = float(sil["buf_max_priority"]), float(sil["buf_alpha"])
    idx, pri = sil["buf_upd2_idx"], sil["buf_upd2_pri"]
    T.update_priorities(t, idx, pri)
    assert np.array_equal(t.sum_tree[1:], sil["buf_sum2"][1:]) and np.array_equal(t.min_tree[1:], sil["buf_min2"][1:])
    assert t.max_priority == float(sil["buf_max_priority2"])
    P = len(t.sum_tree) // 2
    assert t.sum_tree[P + 3] == 1.25 ** t.alpha          # index 3: 7.5, 0.5, then 1.25
    assert t.sum_tree[P + 9] == 1e-6 ** t.alpha          # clamped from below
    # and a path update leaves exactly the tree a full rebuild gives
    s, m = T.rebuild(t.sum_tree[P:], t.min_tree[P:])
    assert np.array_equal(s[1:], t.sum_tree[1:]) and np.array_equal(m[1:], t.min_tree[1:])


def test_first_update_from_the_recorded_batch(sil):
    """buf_sum is itself the result of an update that repeats index 5 (its last priority, 2.5, stays) and
    clamps index 7 from 0 to 1e-6."""
    idx, pri, alpha = sil["buf_upd_idx"], sil["buf_upd_pri"], float(sil["buf_alpha"])
    P = len(sil["buf_sum"]) // 2
    last = {int(i): max(float(p), 1e-6) for i, p in zip(idx, pri)}
    for i, p in last.items():
        assert sil["buf_sum"][P + i] == p ** alpha and sil["buf_min"][P + i] == p ** alpha
    assert last[5] == 2.5 and last[7] == 1e-6


def test_discounted_returns_bitwise(sil):
    for k in range(int(sil["ret_n"])):
        rew, done, g = sil[f"ret{k}_rewards"], sil[f"ret{k}_dones"], float(sil[f"ret{k}_gamma"])
        ref = sil[f"ret{k}_out"]
        assert np.array_equal(np.array(T.discount_with_dones(rew, done, g)), ref)
        # the ring's form of the same chain (R = done ? r : r + gamma R), one env, one append
        n = len(rew)
        ring = T.Ring(n, 1, alpha=1.0, gamma=g)
        ring.step_rollout(np.zeros((n, 1), np.int32), np.zeros((n, 1), np.float32),
                          rew.astype(np.float32).reshape(n, 1), done.astype(np.uint8).reshape(n, 1))
        assert (ring.state == T.ACTIVE).all()
        assert np.array_equal(ring.returns[:, 0], ref.astype(np.float32))


def test_ring_pending_wrap_and_lost_head():
    """N = 2, S = 6, T = 4: env 0 ends an episode in every append, env 1 only after S + 2 steps
    (its head is overwritten while pending and is lost)."""
    S, N, Tn = 6, 2, 4
    ring = T.Ring(S, N, alpha=1.0, gamma=0.5)
    z = np.zeros((Tn, N))
    rew = np.ones((Tn, N), np.float32)
    d = np.zeros((Tn, N), np.uint8)
    d[2, 0] = 1
    ring.step_rollout(z.astype(np.int32), z.astype(np.float32), rew, d)
    assert ring.state[:4, 0].tolist() == [2, 2, 2, 1] and ring.state[:4, 1].tolist() == [1, 1, 1, 1]
    assert ring.returns[:3, 0].tolist() == [1.75, 1.5, 1.0] and ring.n_active == 3
    ring.step_rollout(z.astype(np.int32), z.astype(np.float32), rew, d)  # steps 4, 5, 0, 1 (wraps)
    # env 0: done at ring step 0 (t = 2): step 3 (pending) + 4, 5, 0 become active, step 1 pending
    assert ring.state[:, 0].tolist() == [2, 1, 2, 2, 2, 2]
    assert ring.returns[3, 0] == 1.875 and ring.returns[0, 0] == 1.0
    assert (ring.state[:, 1] == T.PENDING).all()
    d2 = np.zeros((Tn, N), np.uint8)
    d2[0, 1] = 1
    ring.step_rollout(z.astype(np.int32), z.astype(np.float32), rew, d2)  # steps 2, 3, 4, 5
    # env 1: the done at ring step 2 closes what is left of its episode (steps 0, 1, 2: its first steps were
    # overwritten while pending); steps 3..5 are newer than the done and stay pending
    assert ring.state[:, 1].tolist() == [2, 2, 2, 1, 1, 1]
    assert ring.returns[:3, 1].tolist() == [1.75, 1.5, 1.0]
    P = ring.P
    s, m = T.rebuild(ring.sum_tree[P:], ring.min_tree[P:])
    assert np.array_equal(s, ring.sum_tree) and ring.sum_tree[1] == ring.n_active  # alpha = 1, max_priority = 1
    idx, w = ring.sample(np.array([0.0, 0.5, 1.0 - 2.0 ** -53]), 1.0)
    assert all(ring.state[i % S, i // S] == T.ACTIVE for i in idx) and np.array_equal(w, np.ones(3))


def test_loss_twin_cases():
    """delta <= 0: every gradient is zero; delta > 10: no value gradient; rho > 1 + c: no policy gradient
    from that row."""
    logits = np.zeros((4, 3), np.float32)
    lp = np.float32(np.log(1 / 3))
    values = np.array([1.0, 0.0, 0.0, 0.0], np.float32)
    returns = np.array([0.5, 20.0, 1.0, 1.0], np.float32)
    old = np.array([lp, lp, lp - 1.0, lp], np.float32)  # row 2: rho = e > 1.2
    L, mean_a, dz, dv, a, delta = T.sil_loss(logits, values, [0, 1, 2, 0], old, returns, np.ones(4), 0.2, 0.0)
    assert a.tolist() == [0.0, 10.0, 1.0, 1.0] and mean_a == 3.0
    assert not dz[0].any() and dv[0] == 0 and dv[1] == 0 and dv[2] != 0
    assert not dz[2].any() and dz[1].any() and dz[3].any()
    assert np.isfinite(L)
