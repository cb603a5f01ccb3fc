"""TEST INFRASTRUCTURE: plain numpy references of the generic layer kernels
(``csrc/layers.hip``), one function per primitive, and the inputs that the
host and the GPU tests of those kernels share.

No torch op and no GPU is used here.  Inputs are float32; all arithmetic is
float64 unless a function says otherwise (``spmm_seq32_ref`` and
``segment_mean_seq32_ref`` restate the kernel's float32 order of additions and
must be matched bit for bit).  Every float64 result comes with the float64 sum
of the absolute terms of each output element, which ``bound`` turns into the
rounding bound of a float32 evaluation.

``tests/test_layer_ref_host.py`` pins these functions to independent truth
(the oracle's torch_scatter / PyG restatements, torch on the CPU, a
hand-written case); ``tests/test_gpu_layer_kernels.py`` compares the kernels
with them.
"""

from __future__ import annotations

import numpy as np

U32 = 2.0**-24  # unit roundoff of float32
FLT_LOWEST = -np.finfo(np.float32).max
RELU, MEAN, MEAN_CLAMP = 1, 2, 4  # DR_SPMM_* mode bits


def bound(n, sum_abs):
    """A sum of ``n`` products accumulated in float32, by fma or by add,
    differs from the exact sum by at most ``(n + 2) * 2^-24 * sum|terms|``
    (``n - 1`` additions and the final rounding to first order; the spare
    terms cover the second order and a following division or product)."""
    return (np.asarray(n, np.float64) + 2.0) * U32 * sum_abs


# --------------------------------------------------------------------------
# CSR
# --------------------------------------------------------------------------


def csr_ref(row, col, n_rows):
    """Stable CSR of (row, col) by row -> (rowptr [n_rows + 1], perm [E], col[perm])."""
    row = np.asarray(row, np.int64)
    col = np.asarray(col, np.int64)
    rowptr = np.zeros(n_rows + 1, np.int64)
    rowptr[1:] = np.cumsum(np.bincount(row, minlength=n_rows))
    perm = np.argsort(row, kind="stable")
    return rowptr, perm, col[perm]


def _row_reduce(ufunc, rowptr, terms, empty):
    """``ufunc`` over each CSR row of ``terms`` [E, ...]; ``empty`` on empty rows."""
    rowptr = np.asarray(rowptr, np.int64)
    n = rowptr.size - 1
    out = np.full((n, *terms.shape[1:]), empty, dtype=terms.dtype)
    full = rowptr[1:] > rowptr[:-1]
    if full.any():  # between two non-empty rows lie only empty ones: their starts delimit the rows
        out[full] = ufunc.reduceat(terms, rowptr[:-1][full], axis=0)
    return out


def _counts(rowptr):
    rowptr = np.asarray(rowptr, np.int64)
    return rowptr[1:] - rowptr[:-1]


# --------------------------------------------------------------------------
# spmm
# --------------------------------------------------------------------------


def _finish(acc, cnt, mode, dtype):
    """The kernel's mode bits on a row sum ``acc`` [n, C] with row counts ``cnt``."""
    with np.errstate(invalid="ignore", divide="ignore"):
        if mode & MEAN:
            acc = acc / cnt.astype(dtype)[:, None]  # the raw count: 0/0 = NaN on empty rows
        if mode & MEAN_CLAMP:
            acc = acc / np.maximum(cnt, 1).astype(dtype)[:, None]
        if mode & RELU:
            acc = np.where(acc <= 0, dtype(0), acc)  # -0 and negatives -> +0, NaN passes
    return acc


def spmm_ref(rowptr, col, y, w=None, mode=0):
    """``out[i] = sum_{e in row i} w[e] * y[col[e]]`` with the kernel's mode
    bits -> (float64 result, float64 sum of the absolute terms per output,
    after the same division)."""
    y64 = np.asarray(y, np.float64)
    terms = y64[np.asarray(col, np.int64)]
    if w is not None:
        terms = terms * np.asarray(w, np.float64)[:, None]
    cnt = _counts(rowptr)
    acc = _row_reduce(np.add, rowptr, terms, 0.0)
    sabs = _row_reduce(np.add, rowptr, np.abs(terms), 0.0)
    return _finish(acc, cnt, mode, np.float64), _finish(sabs, cnt, mode & ~RELU, np.float64)


def _seq32_rows(rowptr, src_rows, y):
    """float32 row sums of ``y[src_rows]`` over CSR rows, one term at a time in
    CSR order from +0 (every row advances by one term per step)."""
    rowptr = np.asarray(rowptr, np.int64)
    src_rows = np.asarray(src_rows, np.int64)
    y = np.asarray(y, np.float32)
    cnt = _counts(rowptr)
    acc = np.zeros((rowptr.size - 1, y.shape[1]), np.float32)
    order = np.argsort(-cnt, kind="stable")  # rows by falling length: the live ones are a prefix
    live = cnt[order]
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(int(cnt.max()) if cnt.size else 0):
            rows = order[: int(np.searchsorted(-live, -k, side="left"))]  # rows longer than k
            acc[rows] = acc[rows] + y[src_rows[rowptr[rows] + k]]
    return acc, cnt


def spmm_seq32_ref(rowptr, col, y, mode=0):
    """The unweighted row sum in float32, added one edge at a time in CSR
    order; ``MEAN`` divides that float32 sum by the float32 count.  The kernel
    must equal this bit for bit."""
    acc, cnt = _seq32_rows(rowptr, col, y)
    return _finish(acc, cnt, mode, np.float32)


# --------------------------------------------------------------------------
# linear
# --------------------------------------------------------------------------


def xwT_ref(x, w):
    """``y = x w^T`` (x [M, K], w [N, K]) -> (y, |x| |w|^T)."""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    return x @ w.T, np.abs(x) @ np.abs(w).T


def xw_ref(dy, w):
    """``dx = dy w`` (dy [M, N], w [N, K]) -> (dx, |dy| |w|)."""
    dy, w = np.asarray(dy, np.float64), np.asarray(w, np.float64)
    return dy @ w, np.abs(dy) @ np.abs(w)


def dw_ref(dy, x):
    """``dw = dy^T x`` (dy [M, N], x [M, K]) -> (dw [N, K], |dy|^T |x|)."""
    dy, x = np.asarray(dy, np.float64), np.asarray(x, np.float64)
    return dy.T @ x, np.abs(dy).T @ np.abs(x)


def dw_terms(m, n_split):
    """The n of ``bound`` for ``dr_linear_dw``: its longest split range plus
    the ``n_split`` partial planes that are summed."""
    s = np.arange(n_split, dtype=np.int64)
    longest = int(((m * (s + 1)) // n_split - (m * s) // n_split).max())
    return longest + n_split


# --------------------------------------------------------------------------
# vanilla edge MLP + scatter_sum
# --------------------------------------------------------------------------


def _edge_pre(rowptr, col, A, B, ea, wc, be):
    rowptr = np.asarray(rowptr, np.int64)
    col = np.asarray(col, np.int64)
    A, B, be = (np.asarray(t, np.float64) for t in (A, B, be))
    ea = np.asarray(ea, np.float64).reshape(col.size, -1)
    wc = np.asarray(wc, np.float64).reshape(A.shape[1], -1)
    src = np.repeat(np.arange(rowptr.size - 1), _counts(rowptr))
    pre = A[src] + B[col] + ea @ wc.T + be
    pabs = np.abs(A[src]) + np.abs(B[col]) + np.abs(ea) @ np.abs(wc).T + np.abs(be)
    # |pre| within the rounding bound of its own Fe + 3 terms: the float32 gate may fall either way
    unsure = np.abs(pre) <= bound(ea.shape[1] + 3, pabs)
    return src, pre, pabs, unsure


def _transpose_rows(col, n_rows):
    """CSR edge positions grouped by destination (stable) and their row pointer."""
    trowptr, tperm, _ = csr_ref(col, col, n_rows)
    return trowptr, tperm


def edge_mlp_ref(rowptr, col, A, B, ea, wc, be):
    """``S[i, c] = sum_{e in row i} relu(A[i, c] + B[col e, c] + wc[c, :] ea_e + be[c])``.

    ``ea`` [E, Fe] is in CSR order.  Returns a dict: ``S``; ``S_abs`` (the sum
    over the row's edges of |A| + |B| + |wc| |ea| + |be|: with n = Fe + 3 +
    row length it bounds a float32 evaluation); ``min_pre`` (the smallest
    |pre| over the edges of each output, +inf on empty rows) and ``unsure``
    (outputs with an edge whose |pre| lies within its own rounding bound);
    ``S_n`` (the n of ``bound``)."""
    src, pre, pabs, unsure = _edge_pre(rowptr, col, A, B, ea, wc, be)
    return {
        "S": _row_reduce(np.add, rowptr, np.maximum(pre, 0.0), 0.0),
        "S_abs": _row_reduce(np.add, rowptr, pabs, 0.0),
        "min_pre": _row_reduce(np.minimum, rowptr, np.abs(pre), np.inf),
        "unsure": _row_reduce(np.logical_or, rowptr, unsure, False),
        "S_n": np.asarray(ea).reshape(pre.shape[0], -1).shape[1] + 3 + _counts(rowptr)[:, None],
    }


def edge_mlp_bwd_ref(rowptr, col, A, B, ea, wc, be, DS):
    """The backward of ``edge_mlp_ref`` given ``DS = dL/dS``:

    ``D[i] = sum_{e in row i} relu'(pre_e) DS[i]``  (= dL/dA),
    ``DP[j] = sum_{e: col e = j} relu'(pre_e) DS[src e]``  (= dL/dB),
    ``EAP[i, c, f] = sum_{e in row i} relu'(pre_e) DS[i, c] ea_e[f]``,
    with relu' = [pre > 0].  A row without edges has D = EAP = 0 whatever
    DS holds there.  Returns a dict of those, their ``*_abs`` sums, the term
    counts ``*_n`` for ``bound``, ``min_pre`` / ``unsure`` per output row
    (``t_*`` for DP: over the edges arriving at the node)."""
    rowptr = np.asarray(rowptr, np.int64)
    n_rows = rowptr.size - 1
    src, pre, _, unsure = _edge_pre(rowptr, col, A, B, ea, wc, be)
    ea = np.asarray(ea, np.float64).reshape(pre.shape[0], -1)
    fe = ea.shape[1]
    DS = np.asarray(DS, np.float64)
    gate = (pre > 0).astype(np.float64)
    cnt = _row_reduce(np.add, rowptr, gate, 0.0)
    deg = _counts(rowptr)[:, None]
    with np.errstate(invalid="ignore"):
        D = np.where(cnt > 0, DS * cnt, 0.0)
        gea = gate[:, :, None] * ea[:, None, :]  # [E, 32, Fe]
        sea = _row_reduce(np.add, rowptr, gea, 0.0)
        sea_abs = _row_reduce(np.add, rowptr, np.abs(gea), 0.0)
        live = (cnt > 0)[:, :, None]
        EAP = np.where(live, DS[:, :, None] * sea, 0.0)
        EAP_abs = np.where(live, np.abs(DS)[:, :, None] * sea_abs, 0.0)
    trowptr, tperm = _transpose_rows(col, n_rows)
    with np.errstate(invalid="ignore"):
        tterm = np.where(gate[tperm] > 0, DS[src[tperm]], 0.0)  # a closed gate adds nothing, not 0 * DS
    abs_pre = np.abs(pre)
    return {
        "D": D, "D_abs": np.abs(D), "D_n": np.ones_like(D),
        "EAP": EAP.reshape(n_rows, 32, fe), "EAP_abs": EAP_abs, "EAP_n": np.broadcast_to((deg + 1)[:, :, None], EAP.shape),
        "DP": _row_reduce(np.add, trowptr, tterm, 0.0), "DP_abs": _row_reduce(np.add, trowptr, np.abs(tterm), 0.0),
        "DP_n": np.broadcast_to(_counts(trowptr)[:, None], D.shape),
        "min_pre": _row_reduce(np.minimum, rowptr, abs_pre, np.inf), "unsure": _row_reduce(np.logical_or, rowptr, unsure, False),
        "t_min_pre": _row_reduce(np.minimum, trowptr, abs_pre[tperm], np.inf), "t_unsure": _row_reduce(np.logical_or, trowptr, unsure[tperm], False),
    }  # fmt: skip


# --------------------------------------------------------------------------
# segment max / mean
# --------------------------------------------------------------------------


def _segments(dense, n_seg):
    segptr, members, _ = csr_ref(dense, dense, n_seg)
    return segptr, members


def segment_max_ref(dense, x, n_seg, mode):
    """Segment max of ``x`` [n_rows, C] float32 over ``dense`` -> (out float32
    [n_seg, C], arg int64 [n_seg, C]).

    mode 0 (torch_scatter ``scatter_max``): members in index order replace the
    running value, which starts at ``-FLT_MAX``, only when strictly greater:
    the lowest member index wins a tie, NaN (and ``-inf``) never enters, and a
    segment that is empty or was never entered gives out = 0, arg = n_rows.
    mode 1 (``scatter_reduce('amax', include_self=False)``): NaN propagates,
    an empty segment gives 0, an all ``-inf`` segment gives ``-inf``; a zero
    maximum is +0 if any member is +0 (no such mix is tested).  ``arg`` is the
    mode 0 walk's in both modes."""
    x = np.asarray(x, np.float32)
    n_rows = x.shape[0]
    segptr, members = _segments(dense, n_seg)
    xs = x[members]
    with np.errstate(invalid="ignore"):
        valid = xs > np.float32(FLT_LOWEST)  # False for NaN, -inf and -FLT_MAX itself
    vals = np.where(valid, xs, np.float32(-np.inf))
    best = _row_reduce(np.maximum, segptr, vals, np.float32(-np.inf))
    seg_of = np.repeat(np.arange(n_seg), _counts(segptr))
    cand = valid & (vals == best[seg_of])
    arg = _row_reduce(np.minimum, segptr, np.where(cand, members[:, None], n_rows), n_rows)
    won = arg < n_rows
    first = np.take_along_axis(x, np.minimum(arg, max(n_rows - 1, 0)), axis=0) if n_rows else np.zeros_like(best)
    if mode == 0:
        return np.where(won, first, np.float32(0)).astype(np.float32), arg  # the winner's own bits (its zero's sign)
    amax = _row_reduce(np.maximum, segptr, xs, np.float32(0))  # np.maximum propagates NaN
    pos_zero = _row_reduce(np.logical_or, segptr, (xs == 0) & ~np.signbit(xs), False)
    amax = np.where((amax == 0) & pos_zero, np.float32(0), amax)
    amax = np.where((amax == 0) & ~pos_zero & (_counts(segptr)[:, None] > 0), np.float32(-0.0), amax)
    return amax.astype(np.float32), arg


def segment_max_bwd_ref(dense, x, n_seg, mode, dout):
    """float64 ``dx`` of ``segment_max_ref``.  mode 0: ``dout`` goes to the
    arg member alone.  mode 1: ``dout`` is split evenly over the members equal
    to the maximum; torch counts the zero-initialised output as one more tie
    when the maximum is +-0 (the members then share ``dout / (ties + 1)``); a
    NaN maximum equals nothing: 0 * (dout / 0) = NaN on every member."""
    x = np.asarray(x, np.float32)
    dout = np.asarray(dout, np.float64)
    dense = np.asarray(dense, np.int64)
    n_rows = x.shape[0]
    out, arg = segment_max_ref(dense, x, n_seg, mode)
    dx = np.zeros(x.shape, np.float64)
    if mode == 0:
        k, c = np.nonzero(arg < n_rows)
        dx[arg[k, c], c] = dout[k, c]
        return dx
    segptr, members = _segments(dense, n_seg)
    eq = np.zeros(x.shape, np.float64)
    eq[:] = x == out[dense]
    ties = _row_reduce(np.add, segptr, eq[members], 0.0) + (out == 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        share = dout / ties
        dx[:] = eq * share[dense]
    return dx


def segment_mean_ref(dense, x, n_seg):
    """Segment mean with the count clamped to 1 -> (mean, sum of |x| / count)."""
    segptr, members = _segments(dense, n_seg)
    xs = np.asarray(x, np.float64)[members]
    cnt = np.maximum(_counts(segptr), 1).astype(np.float64)[:, None]
    return _row_reduce(np.add, segptr, xs, 0.0) / cnt, _row_reduce(np.add, segptr, np.abs(xs), 0.0) / cnt


def segment_mean_seq32_ref(dense, x, n_seg):
    """The float32 sum in member order divided by the float32 clamped count."""
    segptr, members = _segments(dense, n_seg)
    acc, cnt = _seq32_rows(segptr, members, x)
    return acc / np.maximum(cnt, 1).astype(np.float32)[:, None]


# --------------------------------------------------------------------------
# inputs shared by the host and the GPU tests
# --------------------------------------------------------------------------

EDGE_MLP_SMALL = [(f, fe) for f in (12, 30) for fe in (0, 1, 3, 8)]  # (F, Fe): ld_we = 2F + Fe != Fe
EDGE_MLP_BIG = {"n_rows": 70001, "n_edges": 100000, "f": 4, "fe": 3}  # 70,001 * 32 items: past the grid cap
GATE_CAP = 1e-3  # at most this share of a case's outputs may lie too close to the ReLU gate


def hub_graph(n=300, hub=7, hub_edges=1500, seed=11):
    """The graph of the small cases -> (row, col) int64 in shuffled COO order.

    Directed and asymmetric, about four random edges per node, three self
    loops, four duplicated edges, a hub row of ``hub_edges`` edges (its edge
    ids interleave with the other rows' after the shuffle), nodes 0, 1 and
    n - 1 without any edge, and node 2 with in-edges only."""
    rng = np.random.default_rng(seed)
    inner = np.arange(2, n - 1)  # nodes that may receive edges
    srcs = np.arange(3, n - 1)  # nodes that may send them
    row = rng.choice(srcs, size=4 * n)
    col = rng.choice(inner, size=4 * n)
    loops = rng.choice(srcs, size=3, replace=False)
    dup = rng.choice(row.size, size=4, replace=False)
    hub_col = rng.choice(inner, size=hub_edges)  # with replacement: duplicates inside the hub row too
    row = np.concatenate([row, loops, row[dup], np.full(hub_edges, hub), [hub, 5]])
    col = np.concatenate([col, loops, col[dup], hub_col, [2, 2]])
    order = rng.permutation(row.size)
    return row[order].astype(np.int64), col[order].astype(np.int64)


def sparse_graph(n_rows, n_edges, seed):
    """Random directed multigraph; node 0 and the last node have no edge."""
    rng = np.random.default_rng(seed)
    hi = max(n_rows - 1, 2)
    return rng.integers(1, hi, size=n_edges).astype(np.int64), rng.integers(1, hi, size=n_edges).astype(np.int64)


def edge_mlp_inputs(row, col, n_rows, f, fe, seed):
    """Inputs of one edge-MLP case: A, B [n, 32], ea [E, Fe] in COO order, the
    whole edge weight we [32, 2F + Fe] (``wc`` is its column slice from 2F),
    be with |be| >= 0.05 and a random sign, and DS."""
    rng = np.random.default_rng(seed)
    r32 = lambda *s: rng.standard_normal(s).astype(np.float32)  # noqa: E731
    be = (rng.uniform(0.05, 0.5, 32) * rng.choice([-1.0, 1.0], 32)).astype(np.float32)
    return {"A": r32(n_rows, 32), "B": r32(n_rows, 32), "ea": r32(len(row), fe), "we": 0.3 * r32(32, 2 * f + fe), "be": be, "DS": r32(n_rows, 32)}


def pooling_case(c=7, mode=0, seed=3, extra=0, big=0):
    """Segments with every edge of the two semantics -> (x, dense, n_seg).
    Segment ids: 0 empty, 1 one member, 2 all NaN, 3 all -inf, 4 one NaN among
    finite values, 5 ties, 6 maximum +0, 7 maximum -0, 8 empty, 9 plain,
    10 holds -FLT_MAX and -inf only, 11 (mode 0 only; else empty) -0 before +0,
    12 and 13 empty, then ``extra`` plain segments of 1 to 6 members with
    values on a grid of halves (ties), one segment of ``big`` members if
    ``big``, and two empty trailing segments.  Members are shuffled."""
    rng = np.random.default_rng(seed)
    sizes = {1: 1, 2: 3, 3: 4, 4: 5, 5: 6, 6: 4, 7: 4, 9: 9, 10: 3}
    if mode == 0:
        sizes[11] = 3
    for k in range(extra):
        sizes[14 + k] = int(rng.integers(1, 7))
    if big:
        sizes[14 + extra] = big
    n_seg = 14 + extra + (1 if big else 0) + (2 if extra or big else 0)
    dense = rng.permutation(np.concatenate([np.full(s, k) for k, s in sizes.items()]))
    x = rng.standard_normal((dense.size, c)).astype(np.float32)
    x[dense >= 14] = np.round(2 * x[dense >= 14]) / 2 + np.float32(0)  # + 0: no -0 beside a +0
    x[dense == 2] = np.nan
    x[dense == 3] = -np.inf
    x[np.flatnonzero(dense == 4)[2], :] = np.nan
    x[dense == 5] = np.round(x[dense == 5])  # few distinct values: ties
    x[np.flatnonzero(dense == 5)[[1, 4]], :] = 3.0  # and a tied maximum for certain
    for k, z in ((6, 0.0), (7, -0.0)):
        m = np.flatnonzero(dense == k)
        x[m] = -np.abs(x[m]) - 0.5
        x[m[[1, 3]]] = z
    m = np.flatnonzero(dense == 10)
    x[m] = -np.inf
    x[m[1]] = FLT_LOWEST
    if mode == 0:
        m = np.flatnonzero(dense == 11)
        x[m[0]], x[m[1]], x[m[2]] = -0.0, 0.0, -1.0
    return x, dense.astype(np.int64), n_seg


def assert_same_floats(actual, ref):
    """Equal bit patterns (so the sign of a zero counts), any NaN for a NaN."""
    actual, ref = np.asarray(actual, np.float32), np.asarray(ref, np.float32)
    assert actual.shape == ref.shape, (actual.shape, ref.shape)
    nan = np.isnan(ref)
    np.testing.assert_array_equal(np.isnan(actual), nan)
    np.testing.assert_array_equal(np.ascontiguousarray(actual).view(np.uint32)[~nan], np.ascontiguousarray(ref).view(np.uint32)[~nan])


def assert_within(actual, ref, bnd, skip=None, what=""):
    """|actual - ref| <= bnd elementwise (NaN where ref is NaN, equal where ref
    is infinite), outside ``skip``; prints the worst error in units of its bound."""
    actual, ref = np.asarray(actual, np.float64), np.asarray(ref, np.float64)
    assert actual.shape == ref.shape, (what, actual.shape, ref.shape)
    keep = np.ones(ref.shape, bool) if skip is None else ~np.broadcast_to(skip, ref.shape)
    nan = np.isnan(ref)
    np.testing.assert_array_equal(np.isnan(actual)[keep], nan[keep], err_msg=what)
    ok = keep & ~nan
    a, r, b = actual[ok], ref[ok], np.broadcast_to(bnd, ref.shape)[ok]
    with np.errstate(invalid="ignore"):
        err = np.where(a == r, 0.0, np.abs(a - r))
    bad = ~(err <= b)
    worst = float((err / np.where(b > 0, b, 1.0)).max()) if err.size else 0.0
    print(f"{what}: {err.size} compared, worst error {float(err.max()) if err.size else 0.0:.3e}, at most {worst:.3f} of its bound")
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} outside the bound (worst {worst:.3f} of it)"


def edge_mlp_cases():
    """(name, row, col, n_rows, F, Fe, inputs) of every edge-MLP case of the GPU tests."""
    row, col = hub_graph()
    for f, fe in EDGE_MLP_SMALL:
        yield f"hub-F{f}-Fe{fe}", row, col, 300, f, fe, edge_mlp_inputs(row, col, 300, f, fe, 100 * f + fe)
    b = EDGE_MLP_BIG
    row, col = sparse_graph(b["n_rows"], b["n_edges"], 5)
    yield "gridcap", row, col, b["n_rows"], b["f"], b["fe"], edge_mlp_inputs(row, col, b["n_rows"], b["f"], b["fe"], 6)
