"""GINet input gradients on the tile route
(``attribution.input_gradients(..., tiles=...)`` /
``dr_ginet_large_input_grad_pass``): equal bits with the single-workgroup pass
on graphs both take, the CPU oracle on graphs only the tile route takes, and
the routing around it.

The reference is ``attribution_ref``'s (the oracle GINet in eval mode with
``x`` requiring grad).  Tolerances are the suite's: outputs rtol = atol = 1e-4;
gradients ``_util.assert_grad_close`` (rtol 1e-4, floor 1e-6 max|ref|), per
graph."""

from __future__ import annotations

import functools

import numpy as np
import pytest
import torch
from _util import assert_grad_close

import attribution_ref
import graph_zoo
from attribution_ref import DEV
from attribution_ref import model as _model
from attribution_ref import store as _store
from deeprank2_amd import _lib, attribution
from deeprank2_amd.fused import LDS_MAX, BatchHandle, make_pass
from deeprank2_amd.neuralnets.gnn import ginet
from deeprank2_amd.store import GraphStore, pack_graphs, records_from_batch
from deeprank2_amd.utils.synthetic import make_dataset
from oracle import data_ref

pytestmark = pytest.mark.gpu
TOL = dict(rtol=1e-4, atol=1e-4)
FORMS = {"halos+keys": (True, True), "plain": (False, False)}  # (halos, atomic_max)


def _knob(tile, form):
    halos, atomic_max = FORMS[form]
    return dict(tile=tile, halos=halos, atomic_max=atomic_max)


def _call(batch, name, **kw):
    out_dim, target = attribution_ref.target_of(batch, name)
    key = "seed" if isinstance(target, torch.Tensor) else "target"
    res = attribution.input_gradients(_model(attribution_ref.n_feat(batch), out_dim), _store(batch), **{key: target}, **kw)
    torch.cuda.synchronize()
    return res


@functools.lru_cache(maxsize=None)
def _fused(batch, name):
    """The default call on a named batch: the single-workgroup pass (made once)."""
    res = _call(batch, name)
    assert res.path == "fused"
    return res


@functools.lru_cache(maxsize=None)
def _oracle(batch, name):
    out_dim, target = attribution_ref.target_of(batch, name)
    return attribution_ref.oracle_input_grad(attribution_ref.oracle_model(attribution_ref.n_feat(batch), out_dim), list(attribution_ref.datas(batch)), target)


def _assert_matches_oracle(res, ref, graphs=None, what=""):
    out_o, dx_o, seed_o, off = ref
    graphs = range(len(off) - 1) if graphs is None else graphs
    assert res.dx.shape == dx_o.shape and np.array_equal(res.node_off, off)
    out, dx, seed = res.out.cpu().numpy(), res.dx.cpu().numpy(), res.seed.cpu().numpy()
    for g in graphs:
        np.testing.assert_allclose(out[g], out_o[g], **TOL, err_msg=f"{what} out of graph {g}")
        np.testing.assert_array_equal(seed[g], seed_o[g], err_msg=f"{what} seed of graph {g}")
        assert_grad_close(dx[off[g] : off[g + 1]], dx_o[off[g] : off[g + 1]], err_msg=f"{what} dx of graph {g}")


# --------------------------------------------------------------------------
# 1. equal bits with the single-workgroup pass
# --------------------------------------------------------------------------


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("tile", [16, 64, 128])
@pytest.mark.parametrize("name", ["t1", "seed"])
@pytest.mark.parametrize("batch", attribution_ref.BATCHES)
def test_tile_route_writes_the_single_workgroup_bits(batch, name, tile, form):
    """Short last tiles, clusters straddling tiles, single-tile graphs, N = 1,
    edgeless graphs, a hub, F = 33 (KPT 64, r4(F) = 36) and F = 12."""
    ref = _fused(batch, name)
    res = _call(batch, name, tiles="force", _large=_knob(tile, form))
    assert res.path == "tiles"
    assert torch.equal(res.dx, ref.dx)
    assert torch.equal(res.out, ref.out)
    assert torch.equal(res.seed, ref.seed)


# --------------------------------------------------------------------------
# 2. more than one pass of the (cluster, feature) loop
# --------------------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def _many_clusters(k, seed):
    """Three graphs of about 200 nodes in ``k`` depth-0 clusters, F = 30, with
    seeded normal features (no two nodes alike: the pool has no ties)."""
    graphs = make_dataset(3, seed=seed, n_lo=190, n_hi=210, mean_degree=8.0, k_lo=k, k_hi=k, n_feat=30)
    rng = np.random.default_rng(seed)
    for g in graphs:
        g["x"] = rng.normal(size=g["x"].shape).astype(np.float32)
        assert np.unique(g["x"], axis=0).shape[0] == g["x"].shape[0]
    datas = [data_ref.synthetic_to_data(g, f"k{k}_{j}") for j, g in enumerate(graphs)]
    return GraphStore(pack_graphs(records_from_batch(graph_zoo.batch(datas))), DEV), datas


@pytest.mark.parametrize("form", list(FORMS))
def test_more_items_than_threads_in_the_dz_loop(form):
    store, datas = _many_clusters(40, 91)
    k0 = store._sizes[2]  # noqa: SLF001
    assert int(k0.min()) * 30 > 1024  # K0 F items against 1 024 threads
    model = _model(30, 2)
    res = attribution.input_gradients(model, store, target=1, tiles="force", _large=_knob(64, form))
    assert res.path == "tiles"
    ref = attribution.input_gradients(model, store, target=1)
    if ref.path == "fused":
        assert torch.equal(res.dx, ref.dx) and torch.equal(res.out, ref.out)
    else:
        _assert_matches_oracle(res, attribution_ref.oracle_input_grad(attribution_ref.oracle_model(30, 2), datas, 1), what="K0 = 40")
    assert res.dx.abs().max() > 0


# --------------------------------------------------------------------------
# 3. a graph beyond one workgroup
# --------------------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def _with_large():
    """Three small graphs and one sized from dr_ginet_input_grad_lds_bytes to
    exceed one workgroup's LDS in both forms (degree 8; about N = 1 200), at
    position 2; and the oracle's result for target 1."""
    q = _lib.load().dr_ginet_input_grad_lds_bytes
    n = next(n for n in range(800, 4000, 100) if min(q(n, 6 * n, 30, 4, 12, 1, 1, 2, 0), q(n, 6 * n, 30, 4, 12, 1, 1, 2, 36)) > LDS_MAX + 8 * 1024)
    (big,) = make_dataset(1, seed=81, n_lo=n, n_hi=n, mean_degree=8.0, k_lo=4, k_hi=4)
    small = make_dataset(3, seed=82, n_lo=20, n_hi=60, mean_degree=6.0, k_lo=2, k_hi=13)
    datas = [data_ref.synthetic_to_data(g, f"g{j}") for j, g in enumerate([small[0], small[1], big, small[2]])]
    ref = attribution_ref.oracle_input_grad(attribution_ref.oracle_model(30, 2), datas, 1)
    return GraphStore(pack_graphs(records_from_batch(graph_zoo.batch(datas))), DEV), ref


def _assert_rows_match(res, pos, ref, g, what):
    """Requested graph ``pos`` of ``res`` against graph ``g`` of the oracle's result."""
    off = ref[3]
    assert_grad_close(res.graph(pos).cpu().numpy(), ref[1][off[g] : off[g + 1]], err_msg=f"{what} dx")
    np.testing.assert_allclose(res.out.cpu().numpy()[pos], ref[0][g], **TOL, err_msg=f"{what} out")


def test_graph_beyond_one_workgroup_takes_the_tile_route():
    store, ref = _with_large()
    q = _lib.load().dr_ginet_input_grad_lds_bytes
    alias = int(store.packed.transpose_aliased)
    sizes = store.max_sizes([2])
    for zs in (0, store.agg_x_stride):
        assert q(*sizes[:2], 30, *sizes[2:], alias, 2, zs) > LDS_MAX
    model = _model(30, 2)
    alone = attribution.input_gradients(model, store, indices=[2], target=1, tiles=True)
    assert alone.path == "tiles"
    _assert_rows_match(alone, 0, ref, 2, "the large graph alone")
    mixed = attribution.input_gradients(model, store, batch_size=2, target=1, tiles=True)  # [small, small] fused, [large, small] tiles
    assert mixed.path == "mixed"
    _assert_matches_oracle(mixed, ref, what="mixed")
    # the small graph beside the large one: the single-workgroup pass's bits
    small = attribution.input_gradients(model, store, indices=[3], target=1)
    assert small.path == "fused"
    assert torch.equal(mixed.graph(3), small.dx) and torch.equal(mixed.out[3], small.out[0])
    # the large graph second in its batch: its dZ block starts past row 0
    swapped = attribution.input_gradients(model, store, indices=[1, 2], target=1, tiles=True)
    assert swapped.path == "tiles"
    _assert_rows_match(swapped, 0, ref, 1, "small before large")
    _assert_rows_match(swapped, 1, ref, 2, "large after small")
    assert torch.equal(swapped.graph(1), alone.dx)
    # small graphs stay on the single-workgroup pass, and the default has not moved
    assert attribution.input_gradients(model, store, indices=[0, 1, 3], target=1, tiles=True).path == "fused"
    assert attribution.input_gradients(model, store, indices=[2], target=1).path == "layers"


# --------------------------------------------------------------------------
# 4. the plan survives
# --------------------------------------------------------------------------


@pytest.mark.parametrize("form", list(FORMS))
def test_training_and_attribution_passes_share_one_plan(form):
    """ginet.graph_pass on the tile path, dr_ginet_large_input_grad_pass, and
    the first again, on one handle and one plan: the max keys are back at zero
    and neither pass reads what the other left behind."""
    store, out_dim = _store("asym"), 2
    model = _model(30, out_dim)
    params = [p.detach().contiguous() for p in model.ordered_params()]
    h = BatchHandle(store, np.arange(store.n_graphs, dtype=np.int32))
    h.force_large, h.large_tile = True, 32
    h.large_halos, h.large_atomic_max = FORMS[form]
    f, xs, b = store.n_feat, store.x_stride, h.B
    seed = torch.randn(b, out_dim, generator=torch.Generator().manual_seed(3)).to(DEV)

    def training():
        out = torch.full((b, out_dim), float("nan"), device=DEV)
        slab = torch.full((b * ginet.slab_stride(f),), float("nan"), device=DEV)
        head = torch.zeros(b * ginet.head_stride(out_dim), device=DEV)
        ginet.graph_pass(h, params, out_dim, _lib.DR_PASS_FORWARD | _lib.DR_PASS_BACKWARD, dout=seed, out=out, slab=slab, head=head)
        return out, slab, head

    plan = h.large_plan(out_dim)
    rows = int(store.x.shape[0])
    row_off = torch.from_numpy(np.asarray(store.packed.node_off[:-1], dtype=np.int64).copy()).to(DEV)
    dz = torch.full((rows * (-(-f // 4) * 4),), float("nan"), device=DEV)  # (undefined on entry)

    def attribute():
        out = torch.full((b, out_dim), float("nan"), device=DEV)
        slab = torch.empty(b * ginet.slab_stride(f), device=DEV)
        head = torch.zeros(b * ginet.head_stride(out_dim), device=DEV)
        dx = torch.full((rows, xs), float("nan"), device=DEV)
        p = make_pass(out_dim, _lib.DR_PASS_FORWARD | _lib.DR_PASS_BACKWARD, dout=seed, out=out, slab=slab, head=head)
        ig = _lib.InputGradC()
        ig.dx, ig.row_off, ig.dx_stride = dx.data_ptr(), row_off.data_ptr(), xs
        rc = _lib.load().dr_ginet_large_input_grad_pass(store.cstruct(), h.descs.data_ptr(), b, plan.c, ginet.weights_c(params), p, ig, dz.data_ptr(), plan.conv_lds, plan.tail_lds, _lib.stream_ptr(torch.device(DEV)))
        assert rc == 0
        torch.cuda.synchronize()
        return dx, out

    t1 = training()
    a1 = attribute()
    t2 = training()
    a2 = attribute()
    torch.cuda.synchronize()
    assert h.large_plan(out_dim) is plan
    for u, v in zip(t1, t2):
        assert torch.equal(u, v) and torch.isfinite(u).all()
    for u, v in zip(a1, a2):
        assert torch.equal(u, v) and torch.isfinite(u).all()
    ref = attribution.input_gradients(model, store, seed=seed)
    assert ref.path == "fused" and torch.equal(a1[0][:, :f], ref.dx) and torch.equal(a1[1], ref.out)
    if plan.c.part_key:
        assert not plan.part_key.any()


# --------------------------------------------------------------------------
# 5. bounds
# --------------------------------------------------------------------------


@pytest.mark.parametrize("batch", ["deg", "f33", "f12"])
def test_only_the_requested_rows_are_written(batch):
    store = _store(batch)
    rows, xs, f = int(store.x.shape[0]), store.x_stride, store.n_feat
    buf = torch.full((rows + 64, xs), float("nan"), dtype=torch.float32, device=DEV)
    res = _call(batch, "seed", tiles="force", _large=_knob(16, "halos+keys"), dx_out=buf, batch_size=3)
    assert res.path == "tiles" and res.dx.data_ptr() == buf.data_ptr()
    assert torch.isfinite(buf[:rows]).all()
    assert not buf[:rows, f:].any()  # exact zeros in the pad columns
    assert torch.isnan(buf[rows:]).all()
    assert torch.equal(res.dx, _fused(batch, "seed").dx)


# --------------------------------------------------------------------------
# 6. exact values
# --------------------------------------------------------------------------


def test_rows_without_an_in_edge_are_exactly_zero():
    res = _call("deg", "seed", tiles="force", _large=_knob(64, "plain"))
    assert res.path == "tiles"
    dx = res.dx.cpu().numpy()
    n_zero_rows = 0
    for g, d in enumerate(attribution_ref.datas("deg")):
        rows = dx[res.node_off[g] : res.node_off[g + 1]]
        no_in = np.setdiff1d(np.arange(d.x.shape[0]), d.edge_index.numpy()[1])
        assert not rows[no_in].any(), g
        n_zero_rows += no_in.size
        if g in (0, *graph_zoo.EDGELESS):
            assert no_in.size == d.x.shape[0] and not rows.any()
    assert n_zero_rows > 0 and dx.any()


def test_gradient_is_linear_in_the_seed_exactly():
    out_dim, seed = attribution_ref.target_of("asym", "seed")
    store, model = _store("asym"), _model(30, out_dim)
    one = attribution.input_gradients(model, store, seed=seed, tiles="force")
    two = attribution.input_gradients(model, store, seed=2.0 * seed, tiles="force")
    assert one.path == two.path == "tiles"
    assert torch.equal(two.dx, 2.0 * one.dx) and torch.equal(two.out, one.out)
    assert one.dx.abs().max() > 0


# --------------------------------------------------------------------------
# 7. layer-route fallbacks with tiles=True
# --------------------------------------------------------------------------


def test_more_than_64_clusters_take_the_layer_route():
    store, datas = _many_clusters(70, 92)
    assert int(store._sizes[2].max()) > 64  # noqa: SLF001, PLR2004
    res = attribution.input_gradients(_model(30, 2), store, target=1, tiles=True)
    assert res.path == "layers"
    _assert_matches_oracle(res, attribution_ref.oracle_input_grad(attribution_ref.oracle_model(30, 2), datas, 1), what="K0 = 70")


def test_nonfinite_graph_takes_the_layer_route():
    datas = [d.clone() for d in attribution_ref.datas("asym")]
    datas[3].x[2, 5] = float("nan")
    store = GraphStore(pack_graphs(records_from_batch(graph_zoo.batch(datas))), DEV)
    for tiles in (True, "force"):
        res = attribution.input_gradients(_model(30, 2), store, target=1, tiles=tiles)
        assert res.path == "layers"
        _assert_matches_oracle(res, _oracle("asym", "t1"), graphs=[g for g in range(len(datas)) if g != 3], what=f"beside a non-finite graph, tiles={tiles}")


def test_bf16_store_takes_the_layer_route():
    store = GraphStore(pack_graphs(records_from_batch(graph_zoo.batch(attribution_ref.datas("asym")))), DEV, dtype="bf16")
    for tiles in (True, "force"):
        res = attribution.input_gradients(_model(30, 2), store, target=1, tiles=tiles)
        assert res.path == "layers"
        _assert_matches_oracle(res, _oracle("asym", "t1"), what=f"bf16 store, tiles={tiles}")
