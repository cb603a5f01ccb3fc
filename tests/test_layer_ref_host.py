"""CPU only: pins the numpy references of ``tests/layer_ref.py`` to independent
truth (the oracle's torch_scatter / PyG restatements, torch on the CPU, literal
loops and a hand-written case), and checks for every edge-MLP shape of
``tests/test_gpu_layer_kernels.py`` that the float64 reference alone leaves at
most 0.1 % of the outputs too close to the ReLU gate to be compared."""

from __future__ import annotations

import layer_ref as R
import numpy as np
import pytest
import torch

from oracle import gnn_ref
from oracle import pyg_ops as P


def _loop_segment_max(dense, x, n_seg, mode):
    """The documented semantics, member by member."""
    n, c = x.shape
    out = np.zeros((n_seg, c), np.float32)
    arg = np.full((n_seg, c), n, np.int64)
    for k in range(n_seg):
        mem = np.flatnonzero(dense == k)
        for j in range(c):
            best, a = np.float32(R.FLT_LOWEST), n
            for i in mem:
                if x[i, j] > best:
                    best, a = x[i, j], i
            arg[k, j] = a
            if mode == 0:
                out[k, j] = best if a < n else 0.0
            elif mem.size:
                v = x[mem, j]
                out[k, j] = np.nan if np.isnan(v).any() else v.max()
    return out, arg


@pytest.mark.parametrize("mode", [0, 1])
def test_segment_max_ref_vs_loop(mode):
    x, dense, k = R.pooling_case(mode=mode)
    out, arg = R.segment_max_ref(dense, x, k, mode)
    out_l, arg_l = _loop_segment_max(dense, x, k, mode)
    np.testing.assert_array_equal(arg, arg_l)
    if mode == 0:
        R.assert_same_floats(out, out_l)
    else:  # ndarray.max leaves the sign of a zero maximum open
        np.testing.assert_array_equal(out, out_l)
    assert np.signbit(out[7]).all() and not np.signbit(out[6]).any()
    assert (arg[[0, 2, 3, 8, 10, 12, 13]] == x.shape[0]).all()
    assert (out[[0, 8, 12, 13]] == 0).all()


def test_segment_max_ref_mode0_vs_scatter_max():
    x, dense, k = R.pooling_case(mode=0)
    xt = torch.from_numpy(x).requires_grad_(True)
    out_o, arg_o = P.scatter_max(xt, torch.from_numpy(dense), dim=0, dim_size=k)
    out, arg = R.segment_max_ref(dense, x, k, 0)
    np.testing.assert_array_equal(out, out_o.detach().numpy())
    np.testing.assert_array_equal(arg, arg_o.numpy())
    dout = np.random.default_rng(1).standard_normal(out.shape).astype(np.float32)
    (out_o * torch.from_numpy(dout)).sum().backward()
    dx = R.segment_max_bwd_ref(dense, x, k, 0, dout)
    np.testing.assert_array_equal(dx.astype(np.float32), xt.grad.numpy())
    losers = np.ones(x.shape, bool)
    kk, cc = np.nonzero(arg < x.shape[0])
    losers[arg[kk, cc], cc] = False
    assert (dx[losers] == 0).all()


def test_segment_max_ref_mode1_vs_torch_amax():
    """Values, NaN, the maximum of 0 and its phantom tie against torch's own
    scatter_reduce and its autograd."""
    x, dense, k = R.pooling_case(mode=1)
    xt = torch.from_numpy(x).requires_grad_(True)
    idx = torch.from_numpy(dense).view(-1, 1).expand(-1, x.shape[1])
    out_t = torch.zeros(k, x.shape[1]).scatter_reduce(0, idx, xt, "amax", include_self=False)
    out, _ = R.segment_max_ref(dense, x, k, 1)
    np.testing.assert_array_equal(out, out_t.detach().numpy())
    assert np.isnan(out[2]).all() and np.isnan(out[4]).all() and np.isneginf(out[3]).all()
    dout = np.random.default_rng(2).standard_normal(out.shape).astype(np.float32)
    (out_t * torch.from_numpy(dout)).sum().backward()
    dx = R.segment_max_bwd_ref(dense, x, k, 1, dout)
    np.testing.assert_allclose(dx, xt.grad.numpy(), rtol=1e-6, equal_nan=True)
    # the phantom tie: two members at +-0 share dout / 3, not dout / 2
    for s in (6, 7):
        m = np.flatnonzero(dense == s)
        np.testing.assert_allclose(dx[m[1]], dout[s].astype(np.float64) / 3, rtol=1e-12)
    # and max_pool_x as the networks call it
    out_p, _ = P.max_pool_x(torch.from_numpy(dense), torch.from_numpy(x), torch.zeros(dense.size, dtype=torch.long))
    present = np.unique(dense)
    np.testing.assert_array_equal(out[present], out_p.numpy())


def test_segment_mean_ref_vs_scatter_mean():
    x, dense, k = R.pooling_case(c=3, mode=0)
    x = np.nan_to_num(x, nan=1.5, neginf=-2.0).astype(np.float32)
    x[x == R.FLT_LOWEST] = 0.25
    ref, sabs = R.segment_mean_ref(dense, x, k)
    o = P.scatter_mean(torch.from_numpy(x).double(), torch.from_numpy(dense), dim=0, dim_size=k).numpy()
    np.testing.assert_allclose(ref, o, rtol=1e-14, atol=0)
    assert (ref[[0, 8, 12, 13]] == 0).all()
    o32 = P.scatter_mean(torch.from_numpy(x), torch.from_numpy(dense), dim=0, dim_size=k).numpy()
    seq = R.segment_mean_seq32_ref(dense, x, k)
    assert (np.abs(seq - ref) <= R.bound(np.bincount(dense, minlength=k)[:, None] + 1, sabs)).all()
    np.testing.assert_array_equal(seq, o32)  # torch's CPU scatter_add_ is sequential too


def test_csr_ref_hand_case():
    #            e: 0  1  2  3  4  5
    row = np.array([2, 0, 2, 3, 0, 2])
    col = np.array([1, 3, 0, 3, 1, 1])
    rowptr, perm, cs = R.csr_ref(row, col, 5)  # rows 1 and 4 are empty
    np.testing.assert_array_equal(rowptr, [0, 2, 2, 5, 6, 6])
    np.testing.assert_array_equal(perm, [1, 4, 0, 2, 5, 3])
    np.testing.assert_array_equal(cs, [3, 1, 1, 0, 1, 3])
    rowptr, perm, cs = R.csr_ref(row[:0], col[:0], 3)
    np.testing.assert_array_equal(rowptr, [0, 0, 0, 0])
    assert perm.size == 0 and cs.size == 0


def test_spmm_seq32_ref_vs_index_add():
    """Bit-equal to torch's float32 ``index_add_`` on the CPU, which adds the
    edges in order at this size (2,716 edges, 300 rows, 7 channels)."""
    row, col = R.hub_graph()
    rowptr, perm, cs = R.csr_ref(row, col, 300)
    y = np.random.default_rng(4).standard_normal((300, 7)).astype(np.float32)
    seq = R.spmm_seq32_ref(rowptr, cs, y)
    t = torch.zeros(300, 7).index_add_(0, torch.from_numpy(row), torch.from_numpy(y[col]))
    np.testing.assert_array_equal(seq, t.numpy())
    ref, sabs = R.spmm_ref(rowptr, cs, y)
    assert (np.abs(seq - ref) <= R.bound(np.diff(rowptr)[:, None], sabs)).all()
    # the mode bits
    cnt = np.diff(rowptr)
    mean = R.spmm_seq32_ref(rowptr, cs, y, R.MEAN)
    np.testing.assert_array_equal(np.isnan(mean).all(1), cnt == 0)
    np.testing.assert_array_equal(mean[cnt > 0], seq[cnt > 0] / cnt[cnt > 0, None].astype(np.float32))
    clamp = R.spmm_seq32_ref(rowptr, cs, y, R.MEAN_CLAMP)
    assert (clamp[cnt == 0] == 0).all()
    np.testing.assert_array_equal(clamp[cnt > 0], mean[cnt > 0])
    relu = R.spmm_seq32_ref(rowptr, cs, y, R.RELU)
    np.testing.assert_array_equal(relu, np.maximum(seq, 0))
    assert not np.signbit(relu).any()
    w = np.random.default_rng(5).standard_normal(cs.size).astype(np.float32)
    wref, _ = R.spmm_ref(rowptr, cs, y, w)
    t = torch.zeros(300, 7, dtype=torch.float64).index_add_(0, torch.from_numpy(row), torch.from_numpy((y[col] * w[np.argsort(perm)][:, None].astype(np.float64))))
    np.testing.assert_allclose(wref, t.numpy(), rtol=1e-12, atol=1e-13)


def test_linear_refs():
    rng = np.random.default_rng(6)
    x, w, dy = (rng.standard_normal(s).astype(np.float32) for s in ((9, 5), (4, 5), (9, 4)))
    y, yabs = R.xwT_ref(x, w)
    np.testing.assert_allclose(y, np.einsum("mk,nk->mn", x.astype(np.float64), w.astype(np.float64)), rtol=1e-14)
    np.testing.assert_allclose(yabs, np.einsum("mk,nk->mn", np.abs(x).astype(np.float64), np.abs(w).astype(np.float64)), rtol=1e-14)
    dx, _ = R.xw_ref(dy, w)
    np.testing.assert_allclose(dx, np.einsum("mn,nk->mk", dy.astype(np.float64), w.astype(np.float64)), rtol=1e-14)
    dw, _ = R.dw_ref(dy, x)
    np.testing.assert_allclose(dw, np.einsum("mn,mk->nk", dy.astype(np.float64), x.astype(np.float64)), rtol=1e-14)
    assert R.dw_terms(5, 64) == 1 + 64 and R.dw_terms(257, 3) == 86 + 3 and R.dw_terms(1000, 1) == 1001


@pytest.mark.parametrize("f,fe", [(12, 0), (12, 3), (30, 8)])
def test_edge_mlp_ref_vs_autograd(f, fe):
    """Against autograd through the oracle layer's own three lines (edge MLP on
    [x_a | x_b | ea], scatter_sum by a) in float64."""
    n = 300
    row, col = R.hub_graph()
    rng = np.random.default_rng(7 + fe)
    layer = gnn_ref.VanillaConvolutionalLayer(f, fe).double()
    lin = layer._edge_mlp[0]
    with torch.no_grad():
        lin.bias.copy_(torch.from_numpy(rng.uniform(0.05, 0.5, 32) * rng.choice([-1.0, 1.0], 32)))
    x = torch.from_numpy(rng.standard_normal((n, f))).requires_grad_(True)
    ea = torch.from_numpy(rng.standard_normal((row.size, fe)))
    a, b = torch.from_numpy(row), torch.from_numpy(col)
    # the layer's lines, with the two node products kept as A and B
    A = x @ lin.weight[:, :f].T
    B = x @ lin.weight[:, f : 2 * f].T
    A.retain_grad()
    B.retain_grad()
    m = layer._edge_mlp(torch.cat([x[a], x[b], ea], dim=1))
    s = P.scatter_sum(m, a, dim=0, out=torch.zeros(n, 32, dtype=torch.float64))
    m2 = torch.relu(A[a] + B[b] + ea @ lin.weight[:, 2 * f :].T + lin.bias)
    s2 = P.scatter_sum(m2, a, dim=0, out=torch.zeros(n, 32, dtype=torch.float64))
    np.testing.assert_allclose(s2.detach().numpy(), s.detach().numpy(), rtol=1e-12, atol=1e-12)

    rowptr, perm, cs = R.csr_ref(row, col, n)
    An, Bn = A.detach().numpy(), B.detach().numpy()
    wc = lin.weight.detach().numpy()[:, 2 * f :]
    be = lin.bias.detach().numpy()
    fwd = R.edge_mlp_ref(rowptr, cs, An, Bn, ea.numpy()[perm], wc, be)
    np.testing.assert_allclose(fwd["S"], s.detach().numpy(), rtol=1e-12, atol=1e-12)
    cnt = np.diff(rowptr)
    assert np.isinf(fwd["min_pre"][cnt == 0]).all() and np.isfinite(fwd["min_pre"][cnt > 0]).all()
    assert (fwd["S_abs"] >= fwd["S"]).all()

    DS = rng.standard_normal((n, 32))
    gw, gb, gx = torch.autograd.grad((s * torch.from_numpy(DS)).sum(), [lin.weight, lin.bias, x], retain_graph=True)
    (s2 * torch.from_numpy(DS)).sum().backward()
    DSn = DS.copy()
    DSn[0] = np.nan  # rows without edges: D and EAP are 0 whatever DS holds
    bwd = R.edge_mlp_bwd_ref(rowptr, cs, An, Bn, ea.numpy()[perm], wc, be, DSn)
    np.testing.assert_allclose(bwd["D"], A.grad.numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(bwd["DP"], B.grad.numpy(), rtol=1e-12, atol=1e-12)
    assert (bwd["D"][cnt == 0] == 0).all() and (bwd["EAP"][cnt == 0] == 0).all()
    assert np.abs(bwd["DP"][2]).sum() > 0 and cnt[2] == 0  # node 2: in-edges only
    xn = x.detach().numpy()
    np.testing.assert_allclose(bwd["D"].T @ xn, gw.numpy()[:, :f], rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(bwd["DP"].T @ xn, gw.numpy()[:, f : 2 * f], rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(bwd["EAP"].sum(0), gw.numpy()[:, 2 * f :], rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(bwd["D"].sum(0), gb.numpy(), rtol=1e-10, atol=1e-10)
    W = lin.weight.detach().numpy()
    np.testing.assert_allclose(bwd["D"] @ W[:, :f] + bwd["DP"] @ W[:, f : 2 * f], gx.numpy(), rtol=1e-10, atol=1e-10)


@pytest.mark.parametrize("case", list(R.edge_mlp_cases()), ids=lambda c: c[0])
def test_gate_margin_cap_of_gpu_shapes(case):
    """For every edge-MLP shape of the GPU tests the float64 reference alone
    leaves at most 0.1 % of the outputs within the rounding bound of the gate."""
    _, row, col, n, f, fe, t = case
    rowptr, perm, cs = R.csr_ref(row, col, n)
    wc = t["we"][:, 2 * f :]
    bwd = R.edge_mlp_bwd_ref(rowptr, cs, t["A"], t["B"], t["ea"][perm], wc, t["be"], t["DS"])
    fwd = R.edge_mlp_ref(rowptr, cs, t["A"], t["B"], t["ea"][perm], wc, t["be"])
    np.testing.assert_array_equal(fwd["unsure"], bwd["unsure"])
    for name, flag in (("S/D/EAP", bwd["unsure"]), ("DP", bwd["t_unsure"])):
        share = float(flag.mean())
        print(f"{case[0]} {name}: {int(flag.sum())} of {flag.size} outputs near the gate, smallest |pre| {float(bwd['min_pre'].min()):.3e}")
        assert share <= R.GATE_CAP, (name, share)
