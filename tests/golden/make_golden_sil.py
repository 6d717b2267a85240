#!/usr/bin/env python3
"""Generate tests/golden/sil.npz by RUNNING the parts of the reference's self-imitation code that run
(make_golden.import_reference(); arrays only, no reference source is copied):

  util.SumSegmentTree / MinSegmentTree            util.py:84-215   leaf writes, find_prefixsum_idx
  buffer.PrioritizedReplayBuffer                  buffer.py:397-490, constructed with its intended
                                                  arguments: add / get / update_priorities
  SilModule.discount_with_dones                   sil_module.py:99-105, on an instance made with
                                                  __new__ (its __init__ cannot run, sil_module.py:14)

Run:  python tests/golden/make_golden_sil.py      (does nothing where the reference is absent)
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as G  # noqa: E402


def gen_trees(R, out):
    rs = np.random.RandomState(700)
    for name, P, writes in (("t64", 64, 500), ("t8", 8, 20)):
        st, mt = R.util.SumSegmentTree(P), R.util.MinSegmentTree(P)
        idx = rs.randint(0, P, size=writes)
        val = rs.rand(writes) * 3 + 1e-3
        val[rs.rand(writes) < 0.1] = 0.0  # some leaves written back to empty (sum 0)
        for i, x in zip(idx, val):
            st[int(i)] = float(x)
            mt[int(i)] = float(x) if x > 0 else float("inf")
        out[name + "_sum"] = np.array(st._value, np.float64)
        out[name + "_min"] = np.array(mt._value, np.float64)
        out[name + "_widx"], out[name + "_wval"] = idx.astype(np.int64), val
    # find_prefixsum_idx on a tree whose leaves are all positive
    P = 64
    st = R.util.SumSegmentTree(P)
    leaves = rs.rand(P) + 0.05
    for i in range(P):
        st[i] = float(leaves[i])
    u = np.concatenate([rs.rand(20000), [0.0, 1.0 - 2.0 ** -53]])
    total = st.sum()
    out["pos_sum"] = np.array(st._value, np.float64)
    out["pos_u"] = u
    out["pos_idx"] = np.array([st.find_prefixsum_idx(float(x) * total) for x in u], np.int64)


def gen_buffer(R, out):
    import torch
    rs = np.random.RandomState(701)
    size, alpha, n_add = 40, 0.6, 30
    buf = R.buffer.PrioritizedReplayBuffer(size, 1, G.Box((3,)), G.Discrete(4), alpha)
    for k in range(n_add):
        buf.add(rs.randn(3).astype(np.float32), np.array([k % 4]), torch.tensor([-0.5 - 0.01 * k]), float(k))
    # priorities with a spread, through the reference's own update (float64 values), one index repeated
    idx = np.array(list(range(1, n_add + 1)) + [5, 7, 5], np.int64)
    pri = np.concatenate([rs.rand(n_add) * 4, [0.25, 0.0, 2.5]])
    buf.update_priorities(idx, pri)
    out["buf_cfg"] = np.array([size, n_add], np.int64)
    out["buf_alpha"] = np.float64(alpha)
    out["buf_upd_idx"], out["buf_upd_pri"] = idx, pri
    out["buf_sum"] = np.array(buf.buffer_sum._value, np.float64)
    out["buf_min"] = np.array(buf.buffer_min._value, np.float64)
    out["buf_max_priority"] = np.float64(buf.max_priority)
    for beta in (0.0, 0.4, 1.0):
        np.random.seed(702)
        s = next(buf.get(16, beta))
        tag = f"buf_b{beta:g}_"
        out[tag + "idx"] = s.indexes.numpy().astype(np.int64)
        out[tag + "weights"] = np.asarray(buf.weights, np.float64)  # (left empty by the reference at beta 0)
    # a second update on top: trees after it
    idx2 = np.array([3, 9, 3, 3, 12], np.int64)
    pri2 = np.array([7.5, 1e-9, 0.5, 1.25, 3.0])
    buf.update_priorities(idx2, pri2)
    out["buf_upd2_idx"], out["buf_upd2_pri"] = idx2, pri2
    out["buf_sum2"] = np.array(buf.buffer_sum._value, np.float64)
    out["buf_min2"] = np.array(buf.buffer_min._value, np.float64)
    out["buf_max_priority2"] = np.float64(buf.max_priority)


def gen_returns(R, out):
    import sil_module
    rs = np.random.RandomState(703)
    for k, (n, gamma, dp) in enumerate([(1, 0.99, 0.0), (17, 0.99, 0.2), (200, 0.999, 0.02), (64, 0.9, 1.0)]):
        m = sil_module.SilModule.__new__(sil_module.SilModule)
        m.gamma = gamma
        # float64 values that are float32-representable: the chain is float64 under either numpy promotion rule
        rew = (rs.randn(n) * 2).astype(np.float32).astype(np.float64)
        done = rs.rand(n) < dp
        done[-1] = True
        out[f"ret{k}_gamma"] = np.float64(gamma)
        out[f"ret{k}_rewards"], out[f"ret{k}_dones"] = rew, done
        out[f"ret{k}_out"] = np.array(m.discount_with_dones(list(rew), list(done)), np.float64)
    out["ret_n"] = np.int64(4)


def main():
    if not os.path.isdir(G.REF):
        print("reference not present; the fixture is committed — nothing to do")
        return 0
    R = G.import_reference()
    out = {}
    gen_trees(R, out)
    gen_buffer(R, out)
    gen_returns(R, out)
    G.save("sil", **out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
