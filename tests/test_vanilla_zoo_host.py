"""The VanillaNetwork batches of tests/test_gpu_vanilla_zoo.py, on the CPU:
what that test claims of them holds, and it could tell if it did not.

From the packed arrays and ``vanilla_tile_plan`` on a CPU store, for every
batch of ``vanilla_zoo.BATCHES``:

* the transposed arrays differ from the forward ones (``transpose_aliased``
  false, ``t_col != col`` on every graph whose edge list is asymmetric);
* the 64-row tiles have the sizes recorded in ``vanilla_zoo.STATS``: below the
  2,048 items (256 halo rows) that the chunk kernels' prologues keep in
  registers for the ordinary batches, beyond them in the intended tiles of
  ``dense_tiles``, with no zero offset in its tile records;
* by the kernels' own carve functions (``dr_debug_carve_vanilla_*``) every
  batch expected on the chunk-fused kernels fits 160 KiB, ``hub_tiled`` keeps
  its tile plan but overflows a chunk carve, and ``hub_untiled`` overflows the
  tile carve itself, so ``vanilla_tile_plan`` returns None;
* the network restated in float64 on the planned arrays (columns and
  transposed sources read back through ``halo_ids`` / ``lcol`` / ``ltcol``)
  equals the float64 oracle, and with ``col`` read for ``t_col`` it misses the
  oracle's gradients by more than 100 times the widest GPU tolerance;
* the float32 oracle meets the project's tolerances against the float64
  oracle on every batch and loss, no entry left out (no ReLU gate of these
  batches sits within float32 rounding of zero in a way that shows).

For the per-graph kernel's cases (tests/test_gpu_vanilla_per_graph_widths.py,
tests/test_gpu_multi_output_mse.py):

* every width of ``PER_GRAPH_WIDTHS`` fits ``vanilla_graph_kernel`` by its own
  carve, its store has x rows of r4(F) floats and, at Fe = 0, no
  edge-attribute array; together the widths take every value of the layout
  quantities the kernel derives from F and Fe;
* every parameter's gradient is live at every width (F = 1 under the common
  seed is not: ``vanilla_zoo.SEEDS``);
* ``deg17_2`` leaves siblings of a split graph without rows, by the kernel's
  row split restated;
* the float32 oracle meets the same tolerances with 16 classes and with MSE
  over 3 and 16 outputs, whose last-layer rows from 1 on are exactly zero.
"""

from __future__ import annotations

import numpy as np
import pytest

import vanilla_zoo as V
from deeprank2_amd.fused import LDS_MAX
from deeprank2_amd.neuralnets.gnn.vanilla_gnn import PARAM_NAMES

KPT_ITEMS = 2048  # vanilla_fused.hip: KPT * CT items per workgroup in registers, the rest by the tail loops
ALL = list(V.BATCHES)


@pytest.mark.parametrize("name", ALL)
def test_transposed_arrays_differ_from_forward(name):
    p = V.packed(name)
    assert not p.transpose_aliased
    hard = V.HARD.get(name)
    for g, d in enumerate(V.datas(name)):
        e = slice(int(p.edge_off[g]), int(p.edge_off[g + 1]))
        if V.is_symmetric(d):
            assert g != hard and name not in ("asym", *V.WIDTH_BATCHES)
            continue
        assert not np.array_equal(p.t_col[e], p.col[e]), g
    assert sum(not V.is_symmetric(d) for d in V.datas(name)) >= (2 if hard is not None else 1)


@pytest.mark.parametrize("name", ALL)
def test_tile_sizes_lie_where_the_gpu_test_claims(name):
    _, stats, meta = V.plan(name, lds_check=False)
    assert stats == V.STATS[name]
    n_tiles, hmax, emax, tmax = stats
    assert n_tiles == sum(-(-int(n) // V.CHUNK) for n in V.packed(name).sizes()[0]) == len(meta)
    if name.startswith("dense"):
        first = next(k for k, m in enumerate(meta) if m[7] == V.HARD[name])
        t0, t1, rest = meta[first], meta[first + 1], meta[first + 2 : first + 7]
        # (dr_vanilla_tile: ... 10 ne, 12 nq, 14 n_halo)
        assert t0[10] > KPT_ITEMS and t0[14] * 8 > KPT_ITEMS  # vc_fwd's record and halo tails, HaloV's
        assert t1[12] > KPT_ITEMS and t1[10] < KPT_ITEMS  # EdgeBwd's transposed-record tail alone
        assert all(m[10] < KPT_ITEMS and m[12] < KPT_ITEMS for m in rest)
        assert (emax, tmax) == (t0[10], t1[12]) and hmax == t0[14]
        for k, m in enumerate(meta[first : first + 7]):  # h0, lcol_off, ltcol_off, word0 and the row offsets; e0, q0 past the first tile
            assert all(m[j] > 0 for j in (0, 1, 2, 3, 4, 5, 13, 15, 16)), (k, m)
            assert k == 0 or (m[9] > 0 and m[11] > 0), (k, m)
    elif name.startswith("hub"):
        assert hmax == emax == getattr(V.graph_zoo, name.upper()) + 1  # the hub row's tile: its neighbours and one ordinary edge
    else:
        assert max(emax, tmax, 8 * hmax) < KPT_ITEMS
    if name == "deg" or name in V.HARD:  # a tile without a halo (the single node) beside tiles with one
        assert hmax > 0 and any(m[14] == 0 for m in meta)


@pytest.mark.parametrize("name", ALL)
def test_carves_put_every_batch_on_its_path(name):
    f, fe, _ = V.BATCHES[name]
    stats = V.STATS[name]
    c = V.carve_bytes(f, fe, *stats[1:])
    chunk = max(c["chunk_fwd"], c["chunk_eb2"], c["chunk_eb1"])
    tile = max(c["tile_fwd"], c["tile_bwd"])
    path = V.expected_path(f, fe, True, V.CHUNK, stats)
    assert path == V.PATHS[name]
    assert (V.plan(name) is None) == (tile > LDS_MAX)
    if path == "chunk":
        assert chunk <= LDS_MAX and tile <= LDS_MAX and f <= 32 and fe <= 4  # noqa: PLR2004
    if name == "hub_tiled":  # chunk_fused() falls back to the 64-row tiled edge kernels
        assert tile <= LDS_MAX < chunk
    if name == "hub_untiled":  # vanilla_tile_plan refuses: the untiled kernels
        assert tile > LDS_MAX and stats[1] <= 65535  # noqa: PLR2004
    if name in ("w40_3", "w64_8", "w30_5"):
        assert f > 32 or fe > 4  # noqa: PLR2004
    # the tiles of 16 rows and no tiles: the other kernels of the same batches
    assert V.expected_path(f, fe, True, 0, stats) == V.expected_path(f, fe, False, V.CHUNK, stats) == "untiled"
    if name in ("asym", "deg", "dense3", "dense4"):
        assert V.plan(name, 16) is not None
        assert V.expected_path(f, fe, True, 16, V.plan(name, 16)[1]) == "tiled"


@pytest.mark.parametrize("name", V.WIDTH_BATCHES)
def test_packed_weight_copy_only_within_the_per_graph_kernels_widths(name):
    """dr_vanilla_wpack packs for the per-graph kernel (F <= 32, Fe <= 4) and
    refuses wider models, which always run the pipeline: their spec offers
    FusedTrainStep no packed copy to keep current."""
    import ctypes

    from deeprank2_amd import _lib
    from deeprank2_amd.neuralnets.gnn.vanilla_gnn import make_spec

    f, fe, _ = V.BATCHES[name]
    wide = f > 32 or fe > 4  # noqa: PLR2004
    assert (make_spec(f, fe).wpack is None) == wide
    if wide:  # refused on the host, before any launch
        w, buf = _lib.VanillaWeightsC(), ctypes.create_string_buffer(16)
        assert _lib.load().dr_vanilla_wpack(w, f, fe, ctypes.addressof(buf), None) != 0


def _widest_tolerance(ref):
    return V.GRAD_CEILING * float(np.abs(ref).max()) + 1e-6 + V.GRAD_RTOL * np.abs(ref)


@pytest.mark.parametrize("tile_rows", [64, 16])
@pytest.mark.parametrize("name", ALL)
def test_restated_network_matches_oracle_and_shows_a_mixup(name, tile_rows):
    """The plan's ``lcol`` / ``ltcol`` lead back to ``col`` / ``t_col``; and a
    transposed sum that read ``col`` would be far outside what the GPU test
    tolerates at its widest (1e-5 max|ref| + rtol 1e-4)."""
    state, out_o, loss_o, grads_o = V.oracle(name, "mse", "f64")
    params = [state[n].numpy() for n in PARAM_NAMES]
    cols = V.planned_columns(name, tile_rows)
    out, loss, grads = V.restated(name, params, cols)
    np.testing.assert_allclose(out, out_o.reshape(-1), rtol=0, atol=1e-12)
    assert loss == pytest.approx(loss_o, rel=1e-12)
    for n in PARAM_NAMES:
        np.testing.assert_allclose(grads[n], grads_o[n], rtol=1e-9, atol=1e-12 * max(1.0, float(np.abs(grads_o[n]).max())), err_msg=n)
    _, _, mixed = V.restated(name, params, cols, swap=True)
    miss = max(float((np.abs(mixed[n] - grads_o[n]) / _widest_tolerance(grads_o[n])).max()) for n in PARAM_NAMES)
    assert miss > 100.0, miss  # noqa: PLR2004


@pytest.mark.parametrize(("name", "loss"), [(n, l) for n in ALL for l in V.LOSSES[n]])
def test_float32_oracle_meets_the_tolerances(name, loss):
    """Outputs rtol = atol = 1e-4, loss 1e-4 relative, gradients rtol 1e-4 with
    the floor max(1e-6, 1e-6 max|ref|): every entry."""
    _, out64, loss64, g64 = V.oracle(name, loss, "f64")
    _, out32, loss32, g32 = V.oracle(name, loss, "f32")
    np.testing.assert_allclose(out32, out64, **V.OUT_TOL)
    assert loss32 == pytest.approx(loss64, rel=V.LOSS_RTOL)
    for n in PARAM_NAMES:
        floor = max(1e-6, V.GRAD_NTOL * float(np.abs(g64[n]).max()))
        np.testing.assert_allclose(g32[n], g64[n], rtol=V.GRAD_RTOL, atol=floor, err_msg=n)
        atol, dev = V.grad_atol(g64[n], g32[n])
        assert floor <= atol <= max(floor, V.GRAD_CEILING * float(np.abs(g64[n]).max())) and atol <= max(floor, 4.0 * dev)


# --------------------------------------------------------------------------
# the per-graph kernel's widths (test_gpu_vanilla_per_graph_widths.py)
# --------------------------------------------------------------------------

PER_GRAPH = [f"w{f}_{fe}" for f, fe in V.PER_GRAPH_WIDTHS]
# (name, loss, out_dim) beyond one output and three classes, on the GPU in
# test_gpu_vanilla_per_graph_widths.py and test_gpu_multi_output_mse.py
MULTI_OUT = [(n, "ce", 16) for n in V.CE16] + [(n, "mse", out) for n, out in V.MSE_MULTI]


def _r4(v):
    return (v + 3) & ~3


@pytest.mark.parametrize("name", PER_GRAPH)
def test_per_graph_widths_fit_the_kernel_and_stores_are_as_claimed(name):
    """Every width of ``PER_GRAPH_WIDTHS`` runs on vanilla_graph_kernel: the
    largest graph's carve (dr_vanilla_fused_lds_bytes, a host function) is
    within 160 KiB, the device layout's x rows are r4(F) floats, and a store
    with Fe = 0 carries no edge-attribute array."""
    from deeprank2_amd import _lib
    from deeprank2_amd.fused import BatchHandle
    from deeprank2_amd.neuralnets.gnn import vanilla_gnn as amd
    from deeprank2_amd.store import GraphStore

    f, fe, _ = V.BATCHES[name]
    assert (f, fe) in V.PER_GRAPH_WIDTHS and 1 <= f <= 32 and 0 <= fe <= amd.FUSED_MAX_FE  # noqa: PLR2004
    p = V.packed(name)
    n, e = (int(a.max()) for a in p.sizes()[:2])
    assert n == 130 and p.n_graphs == 4  # noqa: PLR2004
    assert int(_lib.load().dr_vanilla_fused_lds_bytes(n, e, fe)) <= LDS_MAX
    store = GraphStore(p, "cpu")
    assert store.n_feat == f and store.x_stride == _r4(f) and tuple(store.x.shape) == (int(p.sizes()[0].sum()), _r4(f))
    assert not store.x[:, f:].any()  # zero pad columns
    assert store.n_edge_feat == fe and (p.edge_attr is None) == (store.edge_attr is None) == (fe == 0)
    h = BatchHandle(store, np.arange(p.n_graphs))
    for k in (None, 1, 2, 3, 4):
        h.vanilla_split = k
        assert amd.fused_fits(h, f, fe) and (k is None or amd.split_k(h, f, fe) == k)
    h.vanilla_pipeline = True
    assert not amd.fused_fits(h, f, fe) and amd.split_k(h, f, fe) == 1


def test_per_graph_widths_take_every_layout_value():
    """What vanilla_graph.hip derives from F and Fe, over ``PER_GRAPH_WIDTHS``:
    the x row stride, the 16-row and 16-column tile counts of its
    weight-gradient GEMMs (M = F, Nn = F + 33), both states of the packed
    row-pass block's upper half (k = 16 + blk < F), every FE instantiation."""
    fs = {f for f, _ in V.PER_GRAPH_WIDTHS}
    assert {_r4(f) for f in fs} >= {4, 12, 16, 20, 32}
    assert {(f + 15) // 16 for f in fs} == {1, 2} and {15, 16, 17} <= fs
    assert {f + 33 for f in fs} >= {34, 48, 49, 64, 65} and {(f + 33 + 15) // 16 for f in fs} == {3, 4, 5}
    assert {1, 32} <= fs  # every clamp at 0; no pad column
    assert {f > 16 for f in fs} == {True, False} and {16, 17} <= fs
    assert {fe for _, fe in V.PER_GRAPH_WIDTHS} == {0, 1, 2, 3, 4}
    assert min(f for f, fe in V.PER_GRAPH_WIDTHS if fe == 4) == 12 and (1, 0) in V.PER_GRAPH_WIDTHS  # noqa: PLR2004
    assert not set(V.PER_GRAPH_ONLY) & {(f, fe) for f in V.CHUNK_F for fe in V.CHUNK_FE}


@pytest.mark.parametrize("name", PER_GRAPH)
def test_every_gradient_is_live_at_the_per_graph_widths(name):
    """A narrow model can be dead (at F = 1 one ReLU decides a layer): every
    parameter's gradient has non-zero entries, and so has every column block of
    the edge-MLP weights (Wa, Wb, and Wc where Fe > 0) in both layers."""
    f, fe, _ = V.BATCHES[name]
    g = V.oracle(name, "mse", "f64")[3]
    for n in PARAM_NAMES:
        assert np.any(g[n]), n
    for layer in (1, 2):
        we = g[f"_external{layer}._edge_mlp.0.weight"]
        assert we.shape == (32, 2 * f + fe)
        assert np.any(we[:, :f]) and np.any(we[:, f : 2 * f]) and (fe == 0 or np.any(we[:, 2 * f :]))
        wn = g[f"_external{layer}._node_mlp.0.weight"]
        assert np.any(wn[:, :f]) and np.any(wn[:, f:])


@pytest.mark.parametrize(("name", "loss", "out_dim"), MULTI_OUT)
def test_float32_oracle_meets_the_tolerances_with_several_outputs(name, loss, out_dim):
    """``test_float32_oracle_meets_the_tolerances`` for the cases with 16
    classes and with MSE over several outputs; and the multi-output MSE rule:
    the last layer's rows and bias entries from 1 on get exactly zero."""
    _, out64, loss64, g64 = V.oracle(name, loss, "f64", out_dim)
    _, out32, loss32, g32 = V.oracle(name, loss, "f32", out_dim)
    assert out64.shape == (len(V.datas(name)), out_dim)
    np.testing.assert_allclose(out32, out64, **V.OUT_TOL)
    assert loss32 == pytest.approx(loss64, rel=V.LOSS_RTOL)
    for n in PARAM_NAMES:
        floor = max(1e-6, V.GRAD_NTOL * float(np.abs(g64[n]).max()))
        np.testing.assert_allclose(g32[n], g64[n], rtol=V.GRAD_RTOL, atol=floor, err_msg=n)
        atol, dev = V.grad_atol(g64[n], g32[n])
        assert floor <= atol <= max(floor, V.GRAD_CEILING * float(np.abs(g64[n]).max())) and atol <= max(floor, 4.0 * dev)
        assert np.any(g64[n]), n
    w, b = g64["_graph_mlp.2.weight"], g64["_graph_mlp.2.bias"]
    if loss == "mse":
        for g in (g64, g32):
            assert not np.any(g["_graph_mlp.2.weight"][1:]) and not np.any(g["_graph_mlp.2.bias"][1:])
        assert np.any(w[0]) and b[0] != 0
        y = np.array([float(d.y) for d in V.datas(name)])
        assert loss64 == pytest.approx(float(((out64[:, 0] - y) ** 2).sum() / (len(y) * out_dim)), rel=1e-12)
    else:  # every class has a logit gradient of its own
        assert np.abs(w).max(axis=1).min() > 0 and np.all(b != 0)


def _row_bound(rp, n, r, k, rw=16):
    """vanilla_graph.hip's ``row_bound`` restated: the first row i with
    rp[i] + RW i >= ceil(r (E + RW N) / k)."""
    if r <= 0:
        return 0
    if r >= k:
        return n
    t = ((int(rp[n]) + rw * n) * r + k - 1) // k
    return next((i for i in range(n) if int(rp[i]) + rw * i >= t), n)


def test_deg17_2_leaves_siblings_without_rows():
    """The degenerate batch at (17, 2) is the graphs of ``deg`` (same tiles),
    and under the kernel's edge-balanced row split its one-node graph gives
    k - 1 siblings no row at every k > 1 (the two-node graph: k - 2), while
    every graph of the ``w`` batches gives every sibling rows."""
    f, fe, _ = V.BATCHES["deg17_2"]
    p, q = V.packed("deg17_2"), V.packed("deg")
    assert (f, fe) == (17, 2) and p.n_feat == 17 and p.edge_attr.shape[1] == 2  # noqa: PLR2004
    np.testing.assert_array_equal(p.rowptr, q.rowptr)
    np.testing.assert_array_equal(p.col, q.col)
    np.testing.assert_array_equal(p.x, q.x[:, :17])

    def empty_siblings(pk, k):
        out = []
        for g, n in enumerate(int(v) for v in pk.sizes()[0]):
            n0 = int(pk.node_off[g])
            rp = pk.rowptr[n0 + g : n0 + g + n + 1]
            b = [_row_bound(rp, n, r, k) for r in range(k + 1)]
            assert b[0] == 0 and b[-1] == n and all(x <= y for x, y in zip(b, b[1:]))
            out.append(sum(x == y for x, y in zip(b, b[1:])))
        return out

    for k in (2, 3, 4):
        e = empty_siblings(p, k)
        assert e[0] == k - 1 and e[1] == k - 2 and [int(v) for v in p.sizes()[0][:2]] == [1, 2]
        assert not any(empty_siblings(V.packed("w17_2"), k))
