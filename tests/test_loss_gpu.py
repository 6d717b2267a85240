"""The fused PPO loss of csrc/loss.hip (ppox_ppo_loss_*, ppox_ppo_box_loss_*, ppox_minibatch_adv_stats) on
every action-count bucket, past one trip of its 64 x 256 grid, on an index map that is not two powers
of two, on each branch of the max-of-means value loss, sharded over ranks, and refused where it must
be.  Reference: torch-CPU autograd (tests/head_twin.py loss_reference), at the tolerances of
test_ppo_loss_fwd_bwd_vs_torch / test_box_loss_fwd_bwd_vs_torch, which hold the same kernels to the
same reference:
    losses rtol 1e-5 atol 1e-7;  dlogits / dmu rtol 1e-4 atol 1e-5 max|ref|;
    value gradients rtol 1e-5 atol 1e-8;  dlog_std rtol 1e-4 atol 1e-6.
Gradients skip the rows of the reference's edge_mask only (f64 ratio within 1e-5 relative of the clip
range, where the f32 log-prob may fall on the other side of the surrogate's kink); every test asserts
the mask covers at most 0.1 % of its rows.  Every tensor a kernel writes comes out of a sentinel-guarded
Arena (tests/guarded.py), pre-filled with NaN where it must be written in full."""
import numpy as np
import pytest
import torch

import head_twin as H
from guarded import Arena

pytestmark = pytest.mark.gpu

NAN = float("nan")
f32, f64 = torch.float32, torch.float64


def up(a):
    return torch.tensor(np.ascontiguousarray(a)).cuda()


class Dev:
    """A Case on the device, with its advantage moments from ppox_minibatch_adv_stats (one slice of
    `total` = B < T * N rows)."""

    def __init__(self, c, ar):
        import native
        self.roll = {k: up(v) for k, v in c.roll.items()}
        self.idx, self.out, self.values = up(c.idx), up(c.out), up(c.values)
        self.int_values = up(c.int_values) if c.dual else None
        self.log_std = up(c.log_std) if c.box else None
        self.stats = ar.new((1, 4), f64, init=NAN)
        native.minibatch_adv_stats(self.roll["advantages"], self.roll["int_advantages"] if c.dual else None,
                                   self.idx, c.B, c.B, c.T, c.N, self.stats)
        assert not torch.isnan(self.stats).any()


def _rows(c, d, lo, hi):
    """Head outputs and indices of rows [lo, hi); a piece without rows passes null row tensors (an
    empty tensor, whose pointer is null, where the wrapper reads `dual` off int_values)."""
    if hi > lo:
        return d.out[lo:hi], d.values[lo:hi], d.int_values[lo:hi] if c.dual else None, d.idx[lo:hi]
    empty = torch.empty(0, device="cuda")
    assert empty.data_ptr() == 0
    return None, None, empty if c.dual else None, None


def partials(c, d, ar, lo=0, hi=None):
    """ppox_ppo[_box]_loss_partials of rows [lo, hi) into a NaN-prefilled table; all 64 x 8 slots
    must have been written."""
    import native
    hi = c.B if hi is None else hi
    out, v, iv, idx = _rows(c, d, lo, hi)
    tab = ar.new(native.LOSS_PARTIALS * 8, f64, init=NAN)
    if c.box:
        native.ppo_box_loss_partials(out, d.log_std, v, iv, hi - lo, c.D, idx, c.T, c.N, d.roll, d.stats[0], c.clip,
                                     tab)
    else:
        native.ppo_loss_partials(out, v, iv, hi - lo, c.A, idx, c.T, c.N, d.roll, d.stats[0], c.clip, tab)
    assert not torch.isnan(tab).any(), "partials table not fully written"
    t = tab.view(native.LOSS_PARTIALS, 8)
    assert float(t[:, 6].sum()) == hi - lo and not t[:, 7].any()
    return tab


def backward(c, d, ar, table, lo=0, hi=None, accum=None, B_global=None):
    """ppox_ppo[_box]_loss_backward of rows [lo, hi) -> dict of NaN-prefilled outputs, fully written."""
    import native
    hi = c.B if hi is None else hi
    n = hi - lo
    out, v, iv, idx = _rows(c, d, lo, hi)
    w = c.D if c.box else c.A
    g = {"d_out": ar.new((n, w), f32, init=NAN) if n else None, "dv": ar.new(n, f32, init=NAN) if n else None,
         "div": ar.new(n, f32, init=NAN) if n and c.dual else None,
         "accum": ar.new(8, f64, init=0.0) if accum is None else accum}
    Bg = c.B if B_global is None else B_global
    if c.box:
        g["dlsp"] = ar.new(native.LOSS_PARTIALS * c.D, f64, init=NAN)
        g["dls"] = ar.new(c.D, f32, init=NAN)
        native.ppo_box_loss_backward(out, d.log_std, v, iv, n, c.D, idx, c.T, c.N, d.roll, d.stats[0], c.clip, table,
                                     Bg, c.ent_coef, c.vf_coef, c.int_vf_coef, c.scale, g["d_out"], g["dlsp"],
                                     g["dls"], g["dv"], g["div"], g["accum"])
    else:
        native.ppo_loss_backward(out, v, iv, n, c.A, idx, c.T, c.N, d.roll, d.stats[0], c.clip, table, Bg, c.ent_coef,
                                 c.vf_coef, c.int_vf_coef, c.scale, g["d_out"], g["dv"], g["div"], g["accum"])
    torch.cuda.synchronize()
    for k in ("d_out", "dv", "div", "dlsp", "dls"):
        if g.get(k) is not None:
            assert not torch.isnan(g[k]).any(), f"{k} not fully written"
    return g


def check_losses(c, acc, ref, calls=1):
    acc = acc.cpu().numpy()
    for col, key in ((0, "pl"), (1, "vl"), (2, "el"), (3, "loss"), (4, "ivl")):
        np.testing.assert_allclose(acc[col], ref[key], rtol=1e-5, atol=1e-7, err_msg=f"loss_accum[{col}] ({key})")
    assert acc[5] == float(calls) and acc[6] == 0.0 and acc[7] == 0.0


def check_grads(c, g, ref, lo=0, hi=None):
    hi = c.B if hi is None else hi
    if hi == lo:
        return
    edge = ref["edge_mask"]
    assert edge.mean() <= H.EDGE_CAP
    keep = ~edge[lo:hi]
    sg = max(np.abs(ref["d_out"]).max(), 1e-30)
    np.testing.assert_allclose(g["d_out"].cpu().numpy()[keep], ref["d_out"][lo:hi][keep], rtol=1e-4, atol=1e-5 * sg,
                               err_msg="d_out")
    np.testing.assert_allclose(g["dv"].cpu().numpy(), ref["dv"][lo:hi], rtol=1e-5, atol=1e-8, err_msg="dv")
    if c.dual:
        np.testing.assert_allclose(g["div"].cpu().numpy(), ref["div"][lo:hi], rtol=1e-5, atol=1e-8, err_msg="div")


def run_whole(c):
    """One process, one minibatch: partials, backward, every output against the reference."""
    ref = c.reference()
    ar = Arena()
    d = Dev(c, ar)
    g = backward(c, d, ar, partials(c, d, ar))
    ar.check()
    check_losses(c, g["accum"], ref)
    check_grads(c, g, ref)
    if c.box:
        np.testing.assert_allclose(g["dls"].cpu().numpy(), ref["dls"], rtol=1e-4, atol=1e-6, err_msg="dlog_std")
    assert ref["vbranch"] == H.EXPECTED_BRANCH[c.ext]
    if c.dual:
        assert ref["ivbranch"] == H.EXPECTED_BRANCH[c.int_] and c.int_ != c.ext
    return g, ref


# ------------------------------------------------------------------------------------------ buckets
@pytest.mark.parametrize("scale", [1.5, 40.0])
@pytest.mark.parametrize("dual", [False, True])
@pytest.mark.parametrize("A", H.BUCKET_A)
def test_every_action_bucket(A, dual, scale):
    """A = 1, the last A of each MAXA bucket (4 is covered by 2, 8, 18, 32, 64) and the first of the
    next (5, 9, 19, 33), at B = 301 over (T, N) = (7, 53): one and two value heads, plain and
    saturated logits.  The value heads cycle through head_twin.VALUE_PAIRS by A.  Edge rows: 0 of 301
    in each of the 40 cases."""
    run_whole(H.bucket_case(A, dual, scale))


# ------------------------------------------------------------------------ grid stride and index map
@pytest.mark.parametrize("T,N,B,A,dual", [H.STRIDE_SHAPE + (5, True), H.STRIDE_SHAPE + (64, True),
                                          (33, 517, 16385, 5, False), (33, 517, 16385, 18, True)])
def test_grid_stride_and_index_map(T, N, B, A, dual):
    """More rows than the 16,384 threads of the loss grid (one row more, and 257 more), T = 33 and
    N = 517 = 11 x 47 (a swapped T / N or a wrong stride reads other rows), idx the first B of a
    permutation of T x N = 17,061.  The census case (A = 5, B = 16641) holds all five surrogate
    classes (pos_above 1,842, pos_below 5,667, neg_above 1,905, neg_below 5,597, inside 1,630; edge
    rows 0) and is compared class by class."""
    c = H.cat_case(T, N, B, A, dual, 1.5)
    g, ref = run_whole(c)
    if (B, A) == (16641, 5):
        assert all(ref["census"][k] >= 100 for k in H.CLASSES), ref["census"]
        z = c.out.astype(np.float64)
        e = np.exp(z - z.max(1, keepdims=True))
        r = np.exp(np.log(e[np.arange(B), c.rows("actions")] / e.sum(1)) - c.rows("log_probs"))
        got, sg = g["d_out"].cpu().numpy(), np.abs(ref["d_out"]).max()
        above, below = r > 1 + c.clip, r < 1 - c.clip
        for name, m in (("above", above), ("below", below), ("inside", ~above & ~below)):
            m = m & ~ref["edge_mask"]
            assert m.sum() >= 100
            np.testing.assert_allclose(got[m], ref["d_out"][m], rtol=1e-4, atol=1e-5 * sg, err_msg=name)


# ----------------------------------------------------------------------------------- value branches
@pytest.mark.parametrize("ext,int_", H.VALUE_PAIRS + H.TIE_CLIPPED_PAIRS)
@pytest.mark.parametrize("box", [False, True])
def test_value_branches_of_both_heads(ext, int_, box):
    """Each branch of max(mean unclipped, mean clipped) — unclipped larger, clipped larger, exact tie
    (0.5 / 0.5) — on the extrinsic head, with the intrinsic head of the same launch on another one.
    `tie` has no row outside the clip range, so its two halves add up to the full gradient;
    `tie_clipped` has 150 of 301 rows outside it, which keep exactly half."""
    T, N, B = H.BUCKET_SHAPE
    c = H.box_case(T, N, B, 3, True, ext, int_) if box else H.cat_case(T, N, B, 5, True, 1.5, ext, int_)
    g, ref = run_whole(c)
    assert (ref["vbranch"], ref["ivbranch"]) == (H.EXPECTED_BRANCH[ext], H.EXPECTED_BRANCH[int_])
    if ext == "tie":
        assert ref["vmeans"][0] == ref["vmeans"][1]
        # the 0.5 / 0.5 split reproduces the full gradient of one mean: -2 scale vf (ret - v) / B
        full = -2.0 * c.scale * c.vf_coef * (c.rows("returns").astype(np.float64) - c.values) / B
        np.testing.assert_allclose(g["dv"].cpu().numpy(), full, rtol=1e-5, atol=1e-8)
    for kind, key, vals, old, rets, coef in (
            (ext, "dv", c.values, "values", "returns", c.vf_coef),
            (int_, "div", c.int_values, "int_values", "int_returns", c.int_vf_coef)):
        if kind == "tie_clipped":
            full = -2.0 * c.scale * coef * (c.rows(rets).astype(np.float64) - vals) / B
            out = np.abs(vals - c.rows(old)) > c.clip
            assert out.sum() == 2 * (B // 4)
            got = g[key].cpu().numpy()
            np.testing.assert_allclose(got[out], 0.5 * full[out], rtol=1e-5, atol=1e-8)
            np.testing.assert_allclose(got[~out], full[~out], rtol=1e-5, atol=1e-8)
    # single head on the same extrinsic case
    run_whole(H.box_case(T, N, B, 3, False, ext, int_) if box else H.cat_case(T, N, B, 5, False, 1.5, ext, int_))


# --------------------------------------------------------------------------------------- loss_accum
@pytest.mark.parametrize("box", [False, True])
def test_loss_accum_adds_two_minibatches(box):
    """Two different minibatches into one accumulator: columns 0-4 are the sums of the two references'
    pl, vl, el, pl + ent_coef el + vf_coef vl + int_vf_coef ivl, ivl; column 5 is exactly 2."""
    T, N, B = H.BUCKET_SHAPE
    cases = [H.box_case(T, N, B, 2, True, "toward", "away"), H.box_case(T, N, B, 7, True, "away", "tie")] if box \
        else [H.cat_case(T, N, B, 5, True, 1.5, "toward", "away"), H.cat_case(T, N, B, 9, True, 40.0, "away", "tie")]
    ar = Arena()
    accum = ar.new(8, f64, init=0.0)
    want = {k: 0.0 for k in ("pl", "vl", "el", "loss", "ivl")}
    for c in cases:
        d = Dev(c, ar)
        backward(c, d, ar, partials(c, d, ar), accum=accum)
        ref = c.reference()
        total = ref["pl"] + c.ent_coef * ref["el"] + c.vf_coef * ref["vl"] + c.int_vf_coef * ref["ivl"]
        np.testing.assert_allclose(ref["loss"], total, rtol=1e-6)
        for k in want:
            want[k] += ref[k]
    ar.check()
    check_losses(cases[0], accum, want, calls=2)


# ------------------------------------------------------------------------------------------- shards
@pytest.mark.parametrize("split", ["B-1,1", "B,0"])
@pytest.mark.parametrize("dual", [False, True])
@pytest.mark.parametrize("box", [False, True])
def test_two_shards_match_one_process(box, dual, split):
    """One minibatch's rows on two ranks: each writes its own full partials table (a rank without rows
    writes 64 x 8 zeros from null row tensors), the tables are summed as the all-reduce does, each rank
    runs backward on its rows with B_global = B.  Concatenated gradients and every rank's loss_accum
    equal the one-process reference; the Box head's per-rank dlog_std sum to the reference's."""
    T, N, B = H.BUCKET_SHAPE
    c = H.box_case(T, N, B, 7, dual) if box else H.cat_case(T, N, B, 5, dual, 1.5)
    ref = c.reference()
    cut = B - 1 if split == "B-1,1" else B
    pieces = [(0, cut), (cut, B)]
    ar = Arena()
    d = Dev(c, ar)
    tabs = [partials(c, d, ar, lo, hi) for lo, hi in pieces]
    if cut == B:
        assert not tabs[1].any()
    table = ar.new(tabs[0].numel(), f64, init=tabs[0] + tabs[1])
    dls = np.zeros(c.D or 0)
    for lo, hi in pieces:
        g = backward(c, d, ar, table, lo, hi)
        check_losses(c, g["accum"], ref)
        check_grads(c, g, ref, lo, hi)
        if box:
            dls += g["dls"].cpu().numpy().astype(np.float64)
            if hi == lo:
                assert not g["dls"].any() and not g["dlsp"].any()
    ar.check()
    if box:
        np.testing.assert_allclose(dls, ref["dls"], rtol=1e-4, atol=1e-6)


# ----------------------------------------------------------------------------------------- box head
@pytest.mark.parametrize("dual", [False, True])
@pytest.mark.parametrize("D", H.BOX_D)
def test_box_head_every_width(D, dual):
    """D = 1 .. 64 (MAXD) at B = 301 with log_std spanning [-3, 1]: the e * D + d indexing of actions
    and old log-probs, and dlog_std reduced over blocks and waves."""
    run_whole(H.box_bucket_case(D, dual))


def test_box_head_grid_stride_and_census():
    """D = 3 at B = 16641 over (33, 517): the per-thread dlog_std accumulation across grid-stride
    trips.  Census over rows x columns: pos_above 8,029, pos_below 6,855, neg_above 7,863, neg_below
    6,851, inside 20,325; edge elements 0 of 49,923."""
    g, ref = run_whole(H.box_case(*H.STRIDE_SHAPE, 3, True))
    assert all(ref["census"][k] >= 100 for k in H.CLASSES), ref["census"]


# ------------------------------------------------------------------------------ minibatch_adv_stats
@pytest.mark.parametrize("batch", [13, 300])
def test_adv_stats_dual_slices_remainder_and_offset_stream(batch):
    """Both streams over total = 40 * 7 + 3 = 283 of T x N = 7 x 53 rows, in slices of 13 (21 full + a
    remainder of 10) and 300 > 256 threads (one slice of 283: the per-thread loop iterates).  The
    extrinsic stream is centred, the intrinsic one has mean = 100 std.  Reference: two-pass f64 numpy
    on the same f32 data.  Means rtol 1e-12.  Stds rtol n 2^-52 (1 + m^2 / var): the kernel forms
    sum(x^2) - n m^2 in f64, two numbers of size n (var + m^2) each carrying n/2 roundings of 2^-53
    relative at worst, against a difference of (n - 1) var; half of that through the square root.
    Measured on the offset stream: worst 8.5e-13 against 5.2e-11 (n = 13), 1.2e-12 against 7.6e-10
    (n = 283); on the centred one at most 2.2e-16."""
    import native
    T, N, total = 7, 53, 40 * 7 + 3
    rs = np.random.RandomState(batch)
    adv = rs.randn(T, N).astype(np.float32)
    adv -= adv.mean()
    iadv = (100.0 + rs.randn(T, N)).astype(np.float32)
    perm = rs.permutation(T * N)[:total].astype(np.int64)
    nmb = -(-total // batch)
    ar = Arena()
    stats = ar.new((nmb, 4), f64, init=NAN)
    native.minibatch_adv_stats(up(adv), up(iadv), up(perm), total, batch, T, N, stats)
    ar.check()
    st = stats.cpu().numpy()
    assert not np.isnan(st).any()
    for k in range(nmb):
        sl = perm[k * batch:(k + 1) * batch]
        n = len(sl)
        assert n > 1
        for col, src in ((0, adv), (2, iadv)):
            x = src.reshape(-1)[(sl % T) * N + sl // T].astype(np.float64)
            m = x.mean()
            var = ((x - m) ** 2).sum() / (n - 1)
            tol = n * 2.0 ** -52 * (1 + m * m / var)
            print(f"batch={batch} slice={k} col={col}: n={n} mean {st[k, col]:.17g} ref {m:.17g}; "
                  f"std rel err {abs(st[k, col + 1] / np.sqrt(var) - 1):.3g} tol {tol:.3g}")
            np.testing.assert_allclose(st[k, col], m, rtol=1e-12, atol=1e-12 if col == 0 else 0)
            np.testing.assert_allclose(st[k, col + 1], np.sqrt(var), rtol=tol)


# ---------------------------------------------------------------------------------------- refusals
def _refused(fn, *outs):
    import native
    with pytest.raises(native.NativeError):
        fn()
    torch.cuda.synchronize()
    for t in outs:
        if t.dtype == f64 and not torch.isnan(t).any():  # loss_accum: still zero
            assert not t.any()
        else:
            assert torch.isnan(t).all(), "a refused call wrote an output"


@pytest.mark.parametrize("bad", [0, 65])
def test_out_of_range_action_counts_are_refused(bad):
    """A (D) = 0 and 65 return an error from both calls of both heads and launch nothing: the outputs
    keep their NaN prefill, loss_accum its zeros."""
    import native
    T, N, B = 3, 5, 8
    c = H.cat_case(T, N, B, 4, True, 1.5)
    b = H.box_case(T, N, B, 4, True)
    P = native.LOSS_PARTIALS
    ar = Arena()
    for case in (c, b):
        d = Dev(case, ar)
        good = partials(case, d, ar)
        wide = up(np.zeros((B, 65), np.float32))  # rows as wide as the refused count claims
        ls = up(np.zeros(65, np.float32))
        tab = ar.new(P * 8, f64, init=NAN)
        dout, dv, div = ar.new((B, 65), f32, init=NAN), ar.new(B, f32, init=NAN), ar.new(B, f32, init=NAN)
        accum = ar.new(8, f64, init=0.0)
        common = (d.idx, T, N, d.roll, d.stats[0], case.clip)
        if case.box:
            dlsp, dls = ar.new(P * 65, f64, init=NAN), ar.new(65, f32, init=NAN)
            _refused(lambda: native.ppo_box_loss_partials(wide, ls, d.values, d.int_values, B, bad, *common, tab), tab)
            _refused(lambda: native.ppo_box_loss_backward(wide, ls, d.values, d.int_values, B, bad, *common, good, B,
                                                          0.01, 0.5, 0.5, 1.0, dout, dlsp, dls, dv, div, accum),
                     dout, dv, div, dlsp, dls, accum)
        else:
            _refused(lambda: native.ppo_loss_partials(wide, d.values, d.int_values, B, bad, *common, tab), tab)
            _refused(lambda: native.ppo_loss_backward(wide, d.values, d.int_values, B, bad, *common, good, B, 0.01,
                                                      0.5, 0.5, 1.0, dout, dv, div, accum), dout, dv, div, accum)
    ar.check()


@pytest.mark.parametrize("box", [False, True])
def test_b_global_zero_is_refused(box):
    import native
    T, N, B = 3, 5, 8
    c = H.box_case(T, N, B, 4, True) if box else H.cat_case(T, N, B, 4, True, 1.5)
    ar = Arena()
    d = Dev(c, ar)
    tab = partials(c, d, ar)
    with pytest.raises(native.NativeError):
        backward(c, d, ar, tab, B_global=0)
    torch.cuda.synchronize()
    ar.check()
    g = backward(c, d, ar, tab)  # the same call with B_global = B goes through
    ar.check()
    check_losses(c, g["accum"], c.reference())
