"""The generic layer kernels of ``csrc/layers.hip`` one by one against the
plain references of ``tests/layer_ref.py``: CSR build (scan carry, stable
order), spmm and its mode bits, the three linear kernels and the dw splits,
the vanilla edge MLP and its backward, segment max / mean, and every kernel
family once just past the 8192 x 256 grid cap, where only the grid-stride loop
reaches the last work items.

Integer outputs, float32 sums whose order of additions is fixed, maxima and
routed gradients are compared exactly.  Everything else is compared with the
float64 reference within ``layer_ref.bound``: (n + 2) * 2^-24 * sum|terms| per
output element, no rtol / atol.  Edge-MLP outputs with a |pre| within its own
rounding bound of the ReLU gate are left out; their share is asserted to stay
under 0.1 % (``tests/test_layer_ref_host.py`` checks the same on the CPU).

Where a test calls the C ABI itself (parameters the wrappers do not expose,
and all grid-cap cases) the outputs are filled with a sentinel first, so that
an element no work item wrote cannot pass for a right one.
"""

from __future__ import annotations

import functools

import layer_ref as R
import numpy as np
import pytest
import torch

from deeprank2_amd import _lib, ops
from deeprank2_amd.utils import community_pooling as CP

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CAP = 8192 * 256  # grid_for: work items of one sweep of the largest grid
SENT = 1.25e30  # no kernel output of these tests comes near it
ISENT = -7
DR_E_ARG = -1


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _i32(a):
    return _dev(np.asarray(a, np.int32))


def _np(t):
    return t.detach().cpu().numpy()


def _fsent(*shape):
    return torch.full(shape, SENT, dtype=torch.float32, device=DEV)


def _isent(*shape):
    return torch.full(shape, ISENT, dtype=torch.int32, device=DEV)


def _stream():
    return _lib.stream_ptr(torch.device(DEV))


def _past_cap(flat, sentinel):
    """The work items just past one sweep of the capped grid, and the last one, were written."""
    flat = np.asarray(flat).reshape(-1)
    assert flat.size > CAP + 2
    for i in (CAP, CAP + 1, CAP + 255, flat.size - 1):
        assert flat[min(i, flat.size - 1)] != sentinel, f"work item {i} of {flat.size} was never written"


# --------------------------------------------------------------------------
# raw C-ABI calls with sentinel-filled outputs
# --------------------------------------------------------------------------


def c_csr(row, col, n_rows):
    e = row.numel()
    rowptr, perm, cs, scratch = _isent(n_rows + 1), _isent(max(e, 1)), _isent(max(e, 1)), _isent(n_rows + 1)
    rc = _lib.load().dr_csr_from_coo(row.data_ptr(), col.data_ptr(), e, n_rows, rowptr.data_ptr(), perm.data_ptr(), cs.data_ptr(), scratch.data_ptr(), _stream())
    return rc, rowptr, perm[:e], cs[:e]


def c_spmm(rowptr, col, w, y, n_rows, mode):
    out = _fsent(n_rows, y.shape[1])
    rc = _lib.load().dr_spmm_csr_w(rowptr.data_ptr(), col.data_ptr(), _lib.ptr(w), y.data_ptr(), n_rows, y.shape[1], mode, out.data_ptr(), _stream())
    return rc, out


def c_dw(dy, x, n_split):
    (m, n), k = dy.shape, x.shape[1]
    dw, scratch = _fsent(n, k), _fsent(n_split * n * k)
    rc = _lib.load().dr_linear_dw(dy.data_ptr(), x.data_ptr(), m, n, k, dw.data_ptr(), scratch.data_ptr(), n_split, _stream())
    return rc, dw


def c_edge_mlp(g, t, f, fe):
    """dr_edge_mlp_scatter and its backward on an ops.EdgeGraph -> (rc, rc, S, D, DP, EAP)."""
    lib = _lib.load()
    s, d, dp, eap = _fsent(g.n, 32), _fsent(g.n, 32), _fsent(g.n, 32), _fsent(g.n * 32 * max(fe, 1))
    we = t["we"]
    wc = we.data_ptr() + 2 * f * 4
    rc1 = lib.dr_edge_mlp_scatter(g.rowptr.data_ptr(), g.col.data_ptr(), g.n, t["A"].data_ptr(), t["B"].data_ptr(), g.ea.data_ptr(), fe, wc, we.stride(0), t["be"].data_ptr(), s.data_ptr(), _stream())
    rc2 = lib.dr_edge_mlp_scatter_bwd(g.rowptr.data_ptr(), g.col.data_ptr(), g.trowptr.data_ptr(), g.tcol.data_ptr(), g.teid.data_ptr(), g.n, t["A"].data_ptr(), t["B"].data_ptr(), g.ea.data_ptr(), fe, wc, we.stride(0),
                                      t["be"].data_ptr(), t["DS"].data_ptr(), d.data_ptr(), dp.data_ptr(), eap.data_ptr(), _stream())  # fmt: skip
    return rc1, rc2, s, d, dp, eap


def c_segment_max(segptr, members, x, n_seg, mode, with_arg=True):
    n, c = x.shape
    out, arg = _fsent(n_seg, c), _isent(n_seg, c)
    rc = _lib.load().dr_segment_max(segptr.data_ptr(), members.data_ptr(), x.data_ptr(), n_seg, c, n, mode, out.data_ptr(), arg.data_ptr() if with_arg else None, _stream())
    return rc, out, arg


def c_segment_max_bwd(segptr, members, x, out, arg, dout, n_seg, mode):
    n, c = x.shape
    dx = _fsent(n, c)
    rc = _lib.load().dr_segment_max_bwd(segptr.data_ptr(), members.data_ptr(), x.data_ptr(), out.data_ptr(), arg.data_ptr(), dout.data_ptr(), n_seg, c, n, mode, dx.data_ptr(), _stream())
    return rc, dx


def c_segment_mean(segptr, members, x, n_seg):
    out = _fsent(n_seg, x.shape[1])
    rc = _lib.load().dr_segment_mean(segptr.data_ptr(), members.data_ptr(), x.data_ptr(), n_seg, x.shape[1], out.data_ptr(), _stream())
    return rc, out


# --------------------------------------------------------------------------
# shared inputs (computed once, never modified)
# --------------------------------------------------------------------------

N_HUB = 300


@functools.lru_cache(maxsize=None)
def hub():
    """The graph of the small cases and its reference CSR, both ways."""
    row, col = R.hub_graph(N_HUB)
    return {"row": row, "col": col, "csr": R.csr_ref(row, col, N_HUB), "tcsr": R.csr_ref(col, row, N_HUB)}


@functools.lru_cache(maxsize=None)
def big_graph():
    """CAP + 777 edges over 70,001 rows: count / place stride once, and
    70,001 x 32 output elements lie past the cap as well."""
    n, e = 70001, CAP + 777
    row, col = R.sparse_graph(n, e, 21)
    return {"n": n, "row": row, "col": col, "csr": R.csr_ref(row, col, n)}


# --------------------------------------------------------------------------
# CSR build
# --------------------------------------------------------------------------


def _check_csr(got, ref, what):
    for name, g, r in zip(("rowptr", "perm", "col"), got, ref):
        np.testing.assert_array_equal(_np(g).astype(np.int64), r, err_msg=f"{what}: {name}")


@pytest.mark.parametrize("n_rows,n_edges", [(0, 0), (5, 0), (1, 4), (1023, 4092), (1024, 4096), (1025, 4100), (2048, 8192), (3077, 12308)])
def test_csr_from_coo_scan_chunks(n_rows, n_edges):
    """rowptr, perm and col equal the stable reference at one scan chunk, at
    its boundary, at two chunks and at a ragged fourth; both directions."""
    rng = np.random.default_rng(n_rows)
    row = rng.integers(0, max(n_rows, 1), n_edges)
    col = rng.integers(0, max(n_rows, 1), n_edges)
    for r, c, what in ((row, col, "by row"), (col, row, "transposed")):
        _check_csr(ops.csr_from_coo(_dev(r), _dev(c), n_rows), R.csr_ref(r, c, n_rows), what)


def test_csr_hub_graph_order_and_slot_map():
    """A 1,501-edge row whose edge ids interleave with the other rows': the
    per-row sort must restore edge order exactly.  EdgeGraph's slot map sends
    each transposed slot to the CSR slot of the same edge."""
    h = hub()
    ei = _dev(np.stack([h["row"], h["col"]]))
    _check_csr(ops.csr_from_coo(ei[0], ei[1], N_HUB), h["csr"], "by row")
    _check_csr(ops.csr_from_coo(ei[1], ei[0], N_HUB), h["tcsr"], "transposed")
    assert int(np.diff(h["csr"][0]).max()) >= 1500
    ea = np.random.default_rng(1).standard_normal((h["row"].size, 3)).astype(np.float32)
    g = ops.edge_graph(ei, N_HUB, _dev(ea))
    perm, tperm = h["csr"][1], h["tcsr"][1]
    _check_csr((g.rowptr, _dev(perm), g.col), h["csr"], "EdgeGraph")
    np.testing.assert_array_equal(_np(g.trowptr), h["tcsr"][0])
    np.testing.assert_array_equal(_np(g.tcol), h["tcsr"][2])
    np.testing.assert_array_equal(perm[_np(g.teid)], tperm)
    np.testing.assert_array_equal(_np(g.ea), ea[perm])


def test_gridcap_csr_from_coo():
    b = big_graph()
    rc, rowptr, perm, cs = c_csr(_dev(b["row"]), _dev(b["col"]), b["n"])
    assert rc == 0
    perm_h, cs_h = _np(perm), _np(cs)
    _past_cap(perm_h, ISENT)
    _past_cap(cs_h, ISENT)
    # place_kernel's edges past the cap land anywhere: every slot must hold an edge, each edge once
    assert int(np.bincount(perm_h, minlength=perm_h.size).max()) == 1 and perm_h.min() == 0
    np.testing.assert_array_equal(_np(rowptr), b["csr"][0])
    np.testing.assert_array_equal(perm_h, b["csr"][1])
    np.testing.assert_array_equal(cs_h, b["csr"][2])


# --------------------------------------------------------------------------
# spmm
# --------------------------------------------------------------------------


@pytest.mark.parametrize("c", [1, 7, 32, 33])
def test_spmm_sum_and_mean_bit_exact(c):
    h = hub()
    rowptr, _, cs = h["csr"]
    cnt = np.diff(rowptr)
    y = np.random.default_rng(30 + c).standard_normal((N_HUB, c)).astype(np.float32)
    rp, cl, yt = _i32(rowptr), _i32(cs), _dev(y)
    R.assert_same_floats(_np(ops.spmm_csr(rp, cl, yt, N_HUB)), R.spmm_seq32_ref(rowptr, cs, y))
    mean = _np(ops.spmm_csr(rp, cl, yt, N_HUB, mean=True))
    assert (cnt == 0).sum() >= 3 and cnt[0] == 0 and cnt[-1] == 0
    np.testing.assert_array_equal(np.isnan(mean), np.broadcast_to((cnt == 0)[:, None], mean.shape))  # NaN exactly on the empty rows
    R.assert_same_floats(mean, R.spmm_seq32_ref(rowptr, cs, y, R.MEAN))
    rc, clamp = c_spmm(rp, cl, None, yt, N_HUB, R.MEAN_CLAMP)
    assert rc == 0
    clamp = _np(clamp)
    assert (clamp[cnt == 0] == 0).all() and not np.signbit(clamp[cnt == 0]).any()
    R.assert_same_floats(clamp, R.spmm_seq32_ref(rowptr, cs, y, R.MEAN_CLAMP))
    rc, relu = c_spmm(rp, cl, None, yt, N_HUB, R.RELU | R.MEAN_CLAMP)  # the combination sgat.py uses
    assert rc == 0
    R.assert_same_floats(_np(relu), R.spmm_seq32_ref(rowptr, cs, y, R.RELU | R.MEAN_CLAMP))


@pytest.mark.parametrize("c", [1, 7, 32, 33])
def test_spmm_weighted_within_bound(c):
    h = hub()
    rowptr, _, cs = h["csr"]
    cnt = np.diff(rowptr)[:, None]
    rng = np.random.default_rng(40 + c)
    y = rng.standard_normal((N_HUB, c)).astype(np.float32)
    w = rng.standard_normal(cs.size).astype(np.float32)
    rp, cl, yt, wt = _i32(rowptr), _i32(cs), _dev(y), _dev(w)
    for mode, extra in ((0, 0), (R.MEAN_CLAMP, 1), (R.MEAN, 1)):
        rc, out = c_spmm(rp, cl, wt, yt, N_HUB, mode)
        assert rc == 0
        ref, sabs = R.spmm_ref(rowptr, cs, y, w, mode)
        R.assert_within(_np(out), ref, R.bound(cnt + extra, sabs), what=f"spmm_w C={c} mode={mode}")


def test_spmm_relu_nan_and_zero_signs():
    """RELU maps negatives and -0 to +0 and keeps NaN; a row summing -inf gives +0."""
    n, c = 8, 5
    #  row:  0 (pos)  1 (neg)  2 (NaN)  3 (-inf)  4 (-0 by underflow)  5 (+0: y = -0)  6 empty  7 (pos + neg = 0)
    row = np.array([0, 0, 1, 1, 2, 2, 3, 4, 5, 7, 7])
    col = np.array([0, 1, 2, 3, 4, 0, 5, 6, 7, 1, 3])
    y = np.zeros((n, c), np.float32)
    y[0], y[1], y[2], y[3] = 1.5, 0.25, -1.0, -0.25
    y[4], y[5], y[6], y[7] = np.nan, -np.inf, 1e-30, -0.0
    w = np.ones(row.size, np.float32)
    w[7] = -1e-30  # -1e-30 * 1e-30 underflows to -0
    rowptr, perm, cs = R.csr_ref(row, col, n)
    np.testing.assert_array_equal(perm, np.arange(row.size))
    rp, cl, yt, wt = _i32(rowptr), _i32(cs), _dev(y), _dev(w)
    for weights in (None, wt):
        rc, plain = c_spmm(rp, cl, weights, yt, n, 0)
        rc2, relu = c_spmm(rp, cl, weights, yt, n, R.RELU)
        assert rc == 0 and rc2 == 0
        plain, relu = _np(plain), _np(relu)
        assert (plain[0] == 1.75).all() and (plain[1] == -1.25).all() and np.isnan(plain[2]).all() and np.isneginf(plain[3]).all()
        assert (plain[7] == 0).all()
        if weights is not None:
            assert (plain[4] == 0).all() and np.signbit(plain[4]).all()  # the case is live: -0 without RELU
        assert (relu[0] == 1.75).all()
        assert np.isnan(relu[2]).all()
        for r in (1, 3, 5, 6, 7) if weights is None else (1, 3, 4, 5, 6, 7):
            assert (relu[r] == 0).all() and not np.signbit(relu[r]).any(), f"row {r}: {relu[r]}"
    R.assert_same_floats(_np(ops.spmm_csr(rp, cl, yt, n, relu=True)), R.spmm_seq32_ref(rowptr, cs, y, R.RELU))
    rc, out = c_spmm(rp, cl, None, yt, n, R.MEAN | R.MEAN_CLAMP)
    assert rc == DR_E_ARG
    assert (_np(out) == np.float32(SENT)).all()  # and nothing was launched


def test_gridcap_spmm():
    b = big_graph()
    rowptr, _, cs = b["csr"]
    y = np.random.default_rng(50).standard_normal((b["n"], 32)).astype(np.float32)
    rc, out = c_spmm(_i32(rowptr), _i32(cs), None, _dev(y), b["n"], 0)
    assert rc == 0
    out = _np(out)
    _past_cap(out, np.float32(SENT))
    R.assert_same_floats(out, R.spmm_seq32_ref(rowptr, cs, y))


# --------------------------------------------------------------------------
# linear kernels
# --------------------------------------------------------------------------


def _linear_inputs(m, k, n, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(s).astype(np.float32) for s in ((m, k), (n, k), (m, n)))


@pytest.mark.parametrize("m,k,n", [(1, 1, 1), (5, 30, 16), (257, 33, 7), (1000, 16, 32)])
def test_linear_kernels_within_bound(m, k, n):
    x, w, dy = _linear_inputs(m, k, n, 60 + m)
    ref, sabs = R.xwT_ref(x, w)
    R.assert_within(_np(ops.linear_xwT(_dev(x), _dev(w))), ref, R.bound(k, sabs), what=f"xwT {m}x{k}x{n}")
    ref, sabs = R.xw_ref(dy, w)
    R.assert_within(_np(ops.linear_xw(_dev(dy), _dev(w))), ref, R.bound(n, sabs), what=f"xw {m}x{n}x{k}")
    ref, sabs = R.dw_ref(dy, x)
    n_split = max(1, min(64, m // 256))
    R.assert_within(_np(ops.linear_dw(_dev(dy), _dev(x))), ref, R.bound(R.dw_terms(m, n_split), sabs), what=f"dw {m}x{n}x{k}")


def test_linear_kernels_empty_sizes():
    """M = 0 and K = 0 return without error; K = 0 writes zeros."""
    z = lambda *s: torch.zeros(*s, dtype=torch.float32, device=DEV)  # noqa: E731
    assert ops.linear_xwT(z(0, 5), z(3, 5)).shape == (0, 3)
    assert ops.linear_xw(z(0, 3), z(3, 5)).shape == (0, 5)
    dw = ops.linear_dw(z(0, 3), z(0, 5))
    assert dw.shape == (3, 5) and (_np(dw) == 0).all()
    y = ops.linear_xwT(z(4, 0), z(3, 0))
    assert y.shape == (4, 3) and (_np(y) == 0).all()
    assert ops.linear_xw(torch.ones(4, 3, device=DEV), z(3, 0)).shape == (4, 0)
    assert ops.linear_dw(torch.ones(4, 3, device=DEV), z(4, 0)).shape == (3, 0)
    dx = ops.linear_xw(z(4, 0), z(0, 5))  # nothing to sum over
    assert dx.shape == (4, 5) and (_np(dx) == 0).all()
    rc, dw = c_dw(z(0, 3), z(0, 5), 3)
    assert rc == 0 and (_np(dw) == 0).all()


@pytest.mark.parametrize("m", [1, 5, 255, 257, 1000])
@pytest.mark.parametrize("n_split", [1, 3, 64])
def test_linear_dw_splits(n_split, m):
    """Empty ranges (M < n_split), ragged ranges and a single range."""
    n, k = 7, 33
    x, _, dy = _linear_inputs(m, k, n, 70 + m)
    rc, dw = c_dw(_dev(dy), _dev(x), n_split)
    assert rc == 0
    ref, sabs = R.dw_ref(dy, x)
    R.assert_within(_np(dw), ref, R.bound(R.dw_terms(m, n_split), sabs), what=f"dw M={m} n_split={n_split}")


@pytest.mark.parametrize("m", [255, 256, 511, 512, 16384])
def test_linear_dw_wrapper_split_choice(m):
    n, k = 16, 30
    x, _, dy = _linear_inputs(m, k, n, 80)
    ref, sabs = R.dw_ref(dy, x)
    n_split = max(1, min(64, m // 256))
    R.assert_within(_np(ops.linear_dw(_dev(dy), _dev(x))), ref, R.bound(R.dw_terms(m, n_split), sabs), what=f"linear_dw M={m}")


def test_gridcap_linear():
    lib = _lib.load()
    m = 70001
    x, w, _ = _linear_inputs(m, 7, 32, 90)
    y = _fsent(m, 32)
    xt, wt = _dev(x), _dev(w)
    assert lib.dr_linear_xwT(xt.data_ptr(), wt.data_ptr(), m, 7, 32, y.data_ptr(), _stream()) == 0
    _past_cap(_np(y), np.float32(SENT))
    ref, sabs = R.xwT_ref(x, w)
    R.assert_within(_np(y), ref, R.bound(7, sabs), what="xwT past the cap")

    _, w, dy = _linear_inputs(m, 31, 5, 91)  # dy [M, 5], w [5, 31]
    dx = _fsent(m, 31)
    dyt, wt = _dev(dy), _dev(w)
    assert lib.dr_linear_xw(dyt.data_ptr(), wt.data_ptr(), m, 5, 31, dx.data_ptr(), _stream()) == 0
    _past_cap(_np(dx), np.float32(SENT))
    ref, sabs = R.xw_ref(dy, w)
    R.assert_within(_np(dx), ref, R.bound(5, sabs), what="xw past the cap")

    x, _, dy = _linear_inputs(130, 170, 200, 92)  # N * K * n_split = 2,176,000 partial sums
    assert 200 * 170 * 64 > CAP
    rc, dw = c_dw(_dev(dy), _dev(x), 64)
    assert rc == 0
    ref, sabs = R.dw_ref(dy, x)
    R.assert_within(_np(dw), ref, R.bound(R.dw_terms(130, 64), sabs), what="dw past the cap")


# --------------------------------------------------------------------------
# vanilla edge MLP + scatter_sum, and its backward
# --------------------------------------------------------------------------


def _edge_case(name):
    (case,) = [c for c in R.edge_mlp_cases() if c[0] == name]
    _, row, col, n, f, fe, t = case
    t = dict(t)
    t["DS"] = t["DS"].copy()
    t["DS"][0] = np.nan  # node 0 has no edges: D and EAP must be 0 there, not DS * 0
    return row, col, n, f, fe, t


def _check_edge_mlp(s, d, dp, eap, row, col, n, f, fe, t, what):
    rowptr, perm, cs = R.csr_ref(row, col, n)
    cnt = np.diff(rowptr)
    args = (rowptr, cs, t["A"], t["B"], t["ea"][perm], t["we"][:, 2 * f :], t["be"])
    fwd, bwd = R.edge_mlp_ref(*args), R.edge_mlp_bwd_ref(*args, t["DS"])
    skip, tskip = bwd["unsure"], bwd["t_unsure"]
    print(f"{what}: {int(skip.sum())} (by row) and {int(tskip.sum())} (by column) of {skip.size} outputs near the gate, smallest |pre| {float(bwd['min_pre'].min()):.3e}")
    assert skip.mean() <= R.GATE_CAP and tskip.mean() <= R.GATE_CAP
    s, d, dp = _np(s), _np(d), _np(dp)
    eap = _np(eap).reshape(n, 32, max(fe, 1))[:, :, :fe]
    assert cnt[0] == 0 and np.isnan(t["DS"][0]).all()
    for name, a in (("S", s), ("D", d), ("EAP", eap)):  # rows without edges: exactly +0
        assert (a[cnt == 0] == 0).all() and not np.signbit(a[cnt == 0]).any(), f"{what}: {name} on empty rows"
    R.assert_within(s, fwd["S"], R.bound(fwd["S_n"], fwd["S_abs"]), skip, f"{what} S")
    R.assert_within(d, bwd["D"], R.bound(bwd["D_n"], bwd["D_abs"]), skip, f"{what} D")
    R.assert_within(eap, bwd["EAP"], R.bound(bwd["EAP_n"], bwd["EAP_abs"]), skip[:, :, None], f"{what} EAP")
    R.assert_within(dp, bwd["DP"], R.bound(bwd["DP_n"], bwd["DP_abs"]), tskip, f"{what} DP")
    return bwd


@pytest.mark.parametrize("f,fe", R.EDGE_MLP_SMALL)
def test_edge_mlp_scatter_and_backward(f, fe):
    """Fe from 0 to 8 with wc a column slice of we (ld_we = 2F + Fe), self
    loops and duplicates in both walks, a 1,501-edge row, rows without edges
    under a NaN DS, and a node that only receives edges."""
    row, col, n, f, fe, t = _edge_case(f"hub-F{f}-Fe{fe}")
    dt = {k: _dev(v) for k, v in t.items()}
    g = ops.edge_graph(_dev(np.stack([row, col])), n, dt["ea"])
    s = ops.edge_mlp_scatter(g, dt["A"], dt["B"], dt["we"], dt["be"], f, fe)
    d, dp, eap = ops.edge_mlp_scatter_bwd(g, dt["A"], dt["B"], dt["we"], dt["be"], f, fe, dt["DS"])
    bwd = _check_edge_mlp(s, d, dp, eap, row, col, n, f, fe, t, f"edge_mlp F={f} Fe={fe}")
    assert not (row == 2).any() and (col == 2).sum() >= 2 and np.abs(bwd["DP"][2]).sum() > 0  # DP on a node with in-edges only
    assert (row == col).sum() >= 3


def test_edge_mlp_rejects_nine_edge_features():
    row, col, n, f, _, t = _edge_case("hub-F12-Fe8")
    t["ea"] = np.zeros((row.size, 9), np.float32)
    t["we"] = np.zeros((32, 2 * f + 9), np.float32)
    dt = {k: _dev(v) for k, v in t.items()}
    g = ops.edge_graph(_dev(np.stack([row, col])), n, dt["ea"])
    rc1, rc2, s, d, dp, eap = c_edge_mlp(g, dt, f, 9)
    assert rc1 == DR_E_ARG and rc2 == DR_E_ARG
    for o in (s, d, dp, eap):
        assert (_np(o) == np.float32(SENT)).all()
    with pytest.raises(RuntimeError, match="bad argument"):
        ops.edge_mlp_scatter(g, dt["A"], dt["B"], dt["we"], dt["be"], f, 9)


def test_gridcap_edge_mlp():
    row, col, n, f, fe, t = _edge_case("gridcap")
    dt = {k: _dev(v) for k, v in t.items()}
    g = ops.edge_graph(_dev(np.stack([row, col])), n, dt["ea"])
    rc1, rc2, s, d, dp, eap = c_edge_mlp(g, dt, f, fe)
    assert rc1 == 0 and rc2 == 0
    for o in (s, d, dp, eap):
        _past_cap(_np(o), np.float32(SENT))
    _check_edge_mlp(s, d, dp, eap, row, col, n, f, fe, t, "edge_mlp past the cap")


# --------------------------------------------------------------------------
# segment max / mean
# --------------------------------------------------------------------------


def _losers(arg, shape):
    lose = np.ones(shape, bool)
    k, c = np.nonzero(arg < shape[0])
    lose[arg[k, c], c] = False
    return lose


@pytest.mark.parametrize("c", [1, 7, 31])
@pytest.mark.parametrize("mode", [0, 1])
def test_segment_max_semantics_and_backward(mode, c):
    """Empty (interior and trailing), single-member, 1,600-member, all-NaN,
    all -inf, NaN among finite, tied, +0 and -0 maxima; 57 segments."""
    x, dense, n_seg = R.pooling_case(c=c, mode=mode, seed=100 + c, extra=40, big=1600)
    assert n_seg > dense.max() + 1
    n = x.shape[0]
    ref_out, ref_arg = R.segment_max_ref(dense, x, n_seg, mode)
    xa = _dev(x).requires_grad_(True)
    out, arg = CP.segment_max(xa, _dev(dense), n_seg, mode)
    R.assert_same_floats(_np(out), ref_out)
    np.testing.assert_array_equal(_np(arg), ref_arg)
    assert np.signbit(ref_out[7]).all() and (ref_out[6] == 0).all() and not np.signbit(ref_out[6]).any()
    dout = np.random.default_rng(c).standard_normal(ref_out.shape).astype(np.float32)
    (out * _dev(dout)).sum().backward()
    dx = _np(xa.grad)
    ref_dx = R.segment_max_bwd_ref(dense, x, n_seg, mode, dout)
    if mode == 0:
        R.assert_same_floats(dx, ref_dx.astype(np.float32))
        assert (dx[_losers(ref_arg, x.shape)] == 0).all()
    else:
        np.testing.assert_allclose(dx, ref_dx, rtol=1e-6, atol=0, equal_nan=True)
        with np.errstate(invalid="ignore"):
            lost = ~np.isnan(ref_out[dense]) & (x != ref_out[dense])
        assert (dx[lost] == 0).all()
        for s in (6, 7):  # a maximum of +-0: two members and torch's phantom tie share dout
            m = np.flatnonzero(dense == s)
            np.testing.assert_allclose(dx[m[1]], dout[s] / np.float32(3), rtol=1e-6)
    # without arg the forward gives the same values
    segptr, members, _ = R.csr_ref(dense, dense, n_seg)
    rc, out2, arg2 = c_segment_max(_i32(segptr), _i32(members), _dev(x), n_seg, mode, with_arg=False)
    assert rc == 0 and (_np(arg2) == ISENT).all()
    R.assert_same_floats(_np(out2), ref_out)
    assert n == dense.size


@pytest.mark.parametrize("c", [1, 7, 31])
def test_segment_mean(c):
    x, dense, n_seg = R.pooling_case(c=c, mode=0, seed=200 + c, extra=40, big=1600)
    x = np.where(np.isfinite(x) & (x > R.FLT_LOWEST), x, np.float32(0.75)).astype(np.float32)
    out = _np(CP.segment_mean(_dev(x), _dev(dense), n_seg))
    R.assert_same_floats(out, R.segment_mean_seq32_ref(dense, x, n_seg))
    ref, sabs = R.segment_mean_ref(dense, x, n_seg)
    cnt = np.bincount(dense, minlength=n_seg)
    assert (out[cnt == 0] == 0).all()
    R.assert_within(out, ref, R.bound(cnt[:, None] + 1, sabs), what=f"segment_mean C={c}")


@pytest.mark.parametrize("mode", [0, 1])
def test_gridcap_segment_max(mode):
    n_seg, c, n = 70001, 31, 150000
    rng = np.random.default_rng(300)
    dense = rng.integers(0, n_seg - 1, n)
    dense[-1] = n_seg - 1
    x = (np.round(4 * rng.standard_normal((n, c))) / 4 + 0.0).astype(np.float32)  # a grid of quarters: ties (and no -0)
    dout = rng.standard_normal((n_seg, c)).astype(np.float32)
    segptr, members, _ = R.csr_ref(dense, dense, n_seg)
    sp, mb, xt = _i32(segptr), _i32(members), _dev(x)
    rc, out, arg = c_segment_max(sp, mb, xt, n_seg, mode)
    assert rc == 0
    _past_cap(_np(out), np.float32(SENT))
    _past_cap(_np(arg), ISENT)
    ref_out, ref_arg = R.segment_max_ref(dense, x, n_seg, mode)
    R.assert_same_floats(_np(out), ref_out)
    np.testing.assert_array_equal(_np(arg), ref_arg)
    rc, dx = c_segment_max_bwd(sp, mb, xt, out, arg, _dev(dout), n_seg, mode)
    assert rc == 0
    dx = _np(dx)
    assert not (dx == np.float32(SENT)).any()  # every row is a member of some segment
    ref_dx = R.segment_max_bwd_ref(dense, x, n_seg, mode, dout)
    if mode == 0:
        R.assert_same_floats(dx, ref_dx.astype(np.float32))
    else:
        np.testing.assert_allclose(dx, ref_dx, rtol=1e-6, atol=0)


def test_gridcap_segment_mean():
    n_seg, c, n = 70001, 31, 150000
    rng = np.random.default_rng(301)
    dense = rng.integers(0, n_seg - 1, n)
    dense[-1] = n_seg - 1
    x = rng.standard_normal((n, c)).astype(np.float32)
    segptr, members, _ = R.csr_ref(dense, dense, n_seg)
    rc, out = c_segment_mean(_i32(segptr), _i32(members), _dev(x), n_seg)
    assert rc == 0
    _past_cap(_np(out), np.float32(SENT))
    R.assert_same_floats(_np(out), R.segment_mean_seq32_ref(dense, x, n_seg))
