"""GINet integrated gradients on the tile route
(``attribution.integrated_gradients(..., tiles=...)`` /
``dr_ginet_large_integrated_grad_pass``): equal bits with the single-workgroup
pass at the same ``groups`` on graphs both take, the fp64 CPU reference of
``ig_ref`` on a graph only the tile route takes, and the routing around it.

Eight Gauss-Legendre nodes unless a test says otherwise.  Tolerances are the
suite's (``ig_ref``'s docstring): outputs rtol = atol = 1e-4; attributions
``_util.assert_grad_close`` per graph; ``attr_sum`` and ``delta``
``ig_ref.sum_tolerance``."""

from __future__ import annotations

import functools

import numpy as np
import pytest
import torch
from _util import assert_grad_close

import graph_zoo
import ig_ref
import ig_tiles_cases
from attribution_ref import DEV
from attribution_ref import model as _model
from attribution_ref import store as _store
from deeprank2_amd import _lib, attribution
from deeprank2_amd.fused import LDS_MAX, BatchHandle, make_pass
from deeprank2_amd.neuralnets.gnn import ginet
from deeprank2_amd.store import GraphStore, pack_graphs, records_from_batch
from test_gpu_attribution_tiles import FORMS, _knob, _many_clusters

pytestmark = pytest.mark.gpu
FIELDS = ("attr", "out", "out_baseline", "attr_sum", "delta", "seed")


def _baseline(batch, kind, full=False):
    b = ig_ref.baseline_of(batch, kind)
    if b is not None and full:  # the same baseline spelled per node
        b = b.expand(sum(d.x.shape[0] for d in ig_ref.datas(batch)), -1).contiguous()
    return b


def _call(batch, name, kind="zero", full=False, **kw):
    out_dim, target = ig_ref.target_of(batch, name)
    store = _store(batch)
    store.use_agg_x = True
    key = "seed" if isinstance(target, torch.Tensor) else "target"
    res = attribution.integrated_gradients(_model(ig_ref.n_feat(batch), out_dim), store, **{key: target}, baseline=_baseline(batch, kind, full), steps=8, **kw)
    torch.cuda.synchronize()
    return res


@functools.lru_cache(maxsize=None)
def _fused(batch, name, kind, groups):
    """The default call on a named batch: the single-workgroup pass (made once per case, shared, unchanged)."""
    res = _call(batch, name, kind, groups=groups)
    assert res.path == "fused"
    return res


def _assert_equal_bits(res, ref, what=""):
    for k in FIELDS:
        assert torch.equal(getattr(res, k), getattr(ref, k)), (what, k)


# --------------------------------------------------------------------------
# 1. equal bits with the single-workgroup pass
# --------------------------------------------------------------------------


@pytest.mark.parametrize("kind", ig_ref.BASELINES)
@pytest.mark.parametrize("groups", [1, 3, 8])  # 3: ranges of 2 / 3 / 3 steps, one group idles in the last round; 8: one step per group
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("tile", [16, 64, 128])
@pytest.mark.parametrize("name", ["t1", "seed"])
@pytest.mark.parametrize("batch", ig_ref.BATCHES)
def test_tile_route_writes_the_single_workgroup_bits(batch, name, tile, form, groups, kind):
    """N = 1, edgeless graphs, a hub row, short last tiles, clusters straddling
    tiles, single-tile graphs, F = 33 (KPT 64, r4(F) = 36) and F = 12."""
    ref = _fused(batch, name, kind, groups)
    res = _call(batch, name, kind, tiles="force", groups=groups, _large=_knob(tile, form))
    assert res.path == "tiles"
    _assert_equal_bits(res, ref, f"{batch}/{name}/{tile}/{form}/G{groups}/{kind}")
    assert res.attr.abs().max() > 0


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("batch", ig_ref.BATCHES)
def test_mean_baseline_as_a_vector_and_as_a_tensor(batch, form):
    vec = _call(batch, "t1", "mean", tiles="force", groups=3, _large=_knob(64, form))
    full = _call(batch, "t1", "mean", full=True, tiles="force", groups=3, _large=_knob(64, form))
    assert vec.path == full.path == "tiles"
    _assert_equal_bits(full, vec, f"{batch} [rows, F] against [F]")
    _assert_equal_bits(full, _fused(batch, "t1", "mean", 3), f"{batch} [rows, F] against the single-workgroup pass")
    assert not torch.equal(vec.out_baseline, _fused(batch, "t1", "zero", 3).out_baseline)  # a different point


def test_default_groups_on_the_tile_route():
    """The default is IG_TILE_GROUPS_DEFAULT capped by the step count, whatever the batch."""
    g = min(attribution.IG_TILE_GROUPS_DEFAULT, 8)
    res = _call("asym", "t1", tiles="force")
    assert res.path == "tiles"
    _assert_equal_bits(res, _fused("asym", "t1", "zero", g), "default groups")
    alone = attribution.integrated_gradients(_model(30, 2), _store("asym"), indices=[3], target=1, steps=8, tiles="force")
    assert torch.equal(alone.attr, res.graph(3)) and torch.equal(alone.attr_sum[0], res.attr_sum[3])


# --------------------------------------------------------------------------
# 2. the degenerate quadrature is the input-gradient tile pass
# --------------------------------------------------------------------------


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("batch", ["asym", "deg", "f33"])
def test_one_step_at_alpha_one_equals_x_times_input_gradients_bit_for_bit(batch, form):
    out_dim, seed = ig_ref.target_of(batch, "seed")
    store, model = _store(batch), _model(ig_ref.n_feat(batch), out_dim)
    res = attribution.integrated_gradients(model, store, seed=seed, groups=1, tiles="force", _quadrature=([1.0], [1.0]), _large=_knob(64, form))
    grad = attribution.input_gradients(model, store, seed=seed, tiles="force", _large=_knob(64, form))
    assert res.path == grad.path == "tiles" and res.alpha.tolist() == res.weight.tolist() == [1.0]
    assert torch.equal(res.attr, store.x[:, : store.n_feat] * grad.dx)
    assert torch.equal(res.out, grad.out)
    assert res.attr.abs().max() > 0


# --------------------------------------------------------------------------
# 3. more than one pass of the (cluster, feature) chain
# --------------------------------------------------------------------------


@pytest.mark.parametrize("form", list(FORMS))
def test_more_items_than_threads_in_the_dz_chain(form):
    store, datas = _many_clusters(40, 91)
    assert int(store._sizes[2].min()) * 30 > 1024  # noqa: SLF001, PLR2004 (K0 F items against 1 024 threads)
    model = _model(30, 2)
    res = attribution.integrated_gradients(model, store, target=1, steps=8, groups=3, tiles="force", _large=_knob(64, form))
    assert res.path == "tiles"
    ref = attribution.integrated_gradients(model, store, target=1, steps=8, groups=3)
    if ref.path == "fused":
        _assert_equal_bits(res, ref, "K0 = 40")
    else:
        _assert_matches(res, ig_ref.integrated_gradients(ig_ref.oracle_model(30, 2), datas, 1, *ig_ref.nodes(8)), what="K0 = 40")
    assert res.attr.abs().max() > 0


# --------------------------------------------------------------------------
# 4. repeatability, and the plan survives
# --------------------------------------------------------------------------


@pytest.mark.parametrize(("batch", "kind", "form"), [("asym", "zero", "halos+keys"), ("deg", "zero", "plain"), ("f33", "mean", "halos+keys")])
def test_repeated_calls_are_bit_identical(batch, kind, form):
    a = _call(batch, "seed", kind, tiles="force", groups=3, _large=_knob(16, form))
    b = _call(batch, "seed", kind, tiles="force", groups=3, _large=_knob(16, form))
    assert a.path == b.path == "tiles"
    _assert_equal_bits(a, b)
    assert torch.isfinite(a.attr).all()


@pytest.mark.parametrize("form", list(FORMS))
def test_training_and_attribution_passes_share_one_plan(form):
    """ginet.graph_pass on the tile path, dr_ginet_large_integrated_grad_pass
    twice on the same handle and workspaces, and the first again, on one plan:
    every group's max keys are back at zero, the plan's own workspaces were
    left alone, and neither pass reads what the other left behind."""
    store, out_dim, n_steps, n_groups = _store("asym"), 2, 8, 3
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
        torch.cuda.synchronize()
        return out, slab, head

    plan = h.large_plan(out_dim)
    rows = int(store.x.shape[0])
    offs = torch.from_numpy(np.asarray(store.packed.node_off[:-1], dtype=np.int64).copy()).to(DEV)
    quad = torch.from_numpy(np.stack(ig_ref.nodes(n_steps))).to(DEV)
    nan = float("nan")  # (the workspaces are undefined on entry, but for the keys)
    dz = torch.full((n_groups * rows * (-(-f // 4) * 4),), nan, device=DEV)
    z = torch.full((n_groups * rows * xs,), nan, device=DEV)
    keys = torch.zeros(n_groups * b * plan.k0_max * 32, dtype=torch.int64, device=DEV)
    part_val = torch.full((n_groups * plan.n_tiles * plan.k0_max * 32,), nan, device=DEV)
    part_arg = torch.zeros(n_groups * plan.n_tiles * plan.k0_max * 32, dtype=torch.int32, device=DEV)
    part = torch.full((n_groups, rows, xs), nan, device=DEV)
    slab = torch.empty(n_groups * b * ginet.slab_stride(f), device=DEV)
    head = torch.zeros(n_groups * b * ginet.head_stride(out_dim), device=DEV)
    outs = torch.empty(n_groups * b * out_dim, device=DEV)

    def attribute():
        attr = torch.full((rows, xs), nan, device=DEV)
        attr_sum = torch.full((b,), nan, dtype=torch.float64, device=DEV)
        p = make_pass(out_dim, _lib.DR_PASS_FORWARD | _lib.DR_PASS_BACKWARD, dout=seed)
        ig, ws = _lib.IntegratedGradC(), _lib.IgTilesC()
        ig.attr, ig.row_off, ig.dx_stride, ig.n_steps, ig.n_groups = attr.data_ptr(), offs.data_ptr(), xs, n_steps, n_groups
        ig.alpha, ig.weight = quad.data_ptr(), quad.data_ptr() + 4 * n_steps
        ig.part, ig.part_off, ig.part_rows, ig.attr_sum = part.data_ptr(), offs.data_ptr(), rows, attr_sum.data_ptr()
        ig.slab, ig.head, ig.out = slab.data_ptr(), head.data_ptr(), outs.data_ptr()
        ws.dz, ws.z, ws.rows = dz.data_ptr(), z.data_ptr(), rows
        ws.part_key, ws.part_val, ws.part_arg = keys.data_ptr(), part_val.data_ptr(), part_arg.data_ptr()
        rc = _lib.load().dr_ginet_large_integrated_grad_pass(store.cstruct(), h.descs.data_ptr(), b, plan.c, ginet.weights_c(params), p, ig, ws, plan.conv_lds, plan.tail_lds, _lib.stream_ptr(torch.device(DEV)))
        assert rc == 0
        torch.cuda.synchronize()
        return attr, attr_sum

    t1 = training()
    plan_z, plan_val = plan.z.view(torch.int32).clone(), plan.part_val.view(torch.int32).clone()  # (as bits: rows no pass wrote are undefined)
    a1 = attribute()
    assert torch.equal(plan.z.view(torch.int32), plan_z) and torch.equal(plan.part_val.view(torch.int32), plan_val)
    a2 = attribute()
    t2 = training()
    assert h.large_plan(out_dim) is plan
    for u, v in zip(t1, t2):
        assert torch.equal(u, v) and torch.isfinite(u).all()
    for u, v in zip(a1, a2):
        assert torch.equal(u, v) and torch.isfinite(u).all()
    assert not keys.any() and not plan.part_key.any()
    ref = attribution.integrated_gradients(model, store, seed=seed, steps=n_steps, groups=n_groups)
    assert ref.path == "fused" and torch.equal(a1[0][:, :f], ref.attr) and torch.equal(a1[1], ref.attr_sum)
    assert not a1[0][:, f:].any()  # exact zeros in the pad columns


def test_only_the_requested_rows_are_written():
    store = _store("f33")
    rows, xs, f = int(store.x.shape[0]), store.x_stride, store.n_feat
    buf = torch.full((rows + 64, xs), float("nan"), dtype=torch.float32, device=DEV)
    res = _call("f33", "t1", "mean", tiles="force", groups=3, _large=_knob(16, "halos+keys"), attr_out=buf, batch_size=3)
    assert res.path == "tiles" and res.attr.data_ptr() == buf.data_ptr()
    assert torch.isfinite(buf[:rows]).all()
    assert not buf[:rows, f:].any()  # exact zeros in the pad columns
    assert torch.isnan(buf[rows:]).all()
    assert torch.equal(res.attr, _fused("f33", "t1", "mean", 3).attr)  # (a graph's bits do not depend on its batch)


# --------------------------------------------------------------------------
# 5. a graph beyond one workgroup
# --------------------------------------------------------------------------


def _assert_matches(res, ref, graphs=None, pos=None, what=""):
    """Requested graphs of ``res`` (positions ``pos``, default the same) against graphs ``graphs`` of the reference."""
    off = ref["node_off"]
    graphs = list(range(len(off) - 1)) if graphs is None else list(graphs)
    pos = graphs if pos is None else list(pos)
    attr_sum, delta = res.attr_sum.cpu().numpy(), res.delta.cpu().numpy()
    assert attr_sum.dtype == delta.dtype == np.float64
    out, out_b, seed = res.out.cpu().numpy(), res.out_baseline.cpu().numpy(), res.seed.cpu().numpy()
    for i, g in zip(pos, graphs):
        rows = slice(off[g], off[g + 1])
        np.testing.assert_allclose(out[i], ref["out"][g], **ig_ref.TOL, err_msg=f"{what} out of graph {g}")
        np.testing.assert_allclose(out_b[i], ref["out_baseline"][g], **ig_ref.TOL, err_msg=f"{what} out_baseline of graph {g}")
        np.testing.assert_array_equal(seed[i], ref["seed"][g], err_msg=f"{what} seed of graph {g}")
        assert_grad_close(res.graph(i).cpu().numpy(), ref["attr"][rows], err_msg=f"{what} attr of graph {g}")
        tol = ig_ref.sum_tolerance(ref, g)
        assert abs(attr_sum[i] - ref["attr_sum"][g]) <= tol, (what, g, attr_sum[i], ref["attr_sum"][g], tol)
        assert abs(delta[i] - ref["delta"][g]) <= tol, (what, g, delta[i], ref["delta"][g], tol)


@functools.lru_cache(maxsize=None)
def _large_store():
    return GraphStore(pack_graphs(records_from_batch(graph_zoo.batch(ig_tiles_cases.datas()))), DEV)


def _large_call(kind="zero", **kw):
    res = attribution.integrated_gradients(_model(ig_tiles_cases.F, ig_tiles_cases.OUT_DIM), _large_store(), target=ig_tiles_cases.TARGET, baseline=ig_tiles_cases.baseline(kind), steps=ig_tiles_cases.STEPS, **kw)
    torch.cuda.synchronize()
    return res


def test_the_large_graph_exceeds_one_workgroup_in_the_z_form():
    store = _large_store()
    sizes = store.max_sizes([ig_tiles_cases.LARGE_AT])
    q = _lib.load().dr_ginet_integrated_grad_lds_bytes
    assert q(*sizes[:2], 30, *sizes[2:], int(store.packed.transpose_aliased), 2, store.agg_x_stride) > LDS_MAX
    for g in (0, 1, 3):
        sizes = store.max_sizes([g])
        assert q(*sizes[:2], 30, *sizes[2:], int(store.packed.transpose_aliased), 2, store.agg_x_stride) <= LDS_MAX


@pytest.mark.parametrize("groups", [1, 3])
def test_graph_beyond_one_workgroup_takes_the_tile_route(groups):
    ref = ig_tiles_cases.reference()
    together = _large_call(tiles=True, groups=groups)
    assert together.path == "tiles"
    _assert_matches(together, ref, what=f"one batch, G = {groups}")
    apart = _large_call(tiles=True, groups=groups, batch_size=2)  # [small, small] single-workgroup, [large, small] tiles
    assert apart.path == "mixed"
    _assert_matches(apart, ref, what=f"batches of two, G = {groups}")
    # the large graph's bits do not depend on its batch
    assert torch.equal(apart.graph(2), together.graph(2)) and torch.equal(apart.attr_sum[2], together.attr_sum[2])
    assert together.graph(2).abs().max() > 0


def test_graph_beyond_one_workgroup_with_a_mean_baseline():
    res = _large_call("mean", tiles=True, groups=3)
    assert res.path == "tiles"
    _assert_matches(res, ig_tiles_cases.reference("mean"), what="mean baseline")
    full = ig_tiles_cases.baseline("mean").expand(int(_large_store().x.shape[0]), -1).contiguous()
    per_node = attribution.integrated_gradients(_model(30, 2), _large_store(), target=1, baseline=full, steps=8, groups=3, tiles=True)
    _assert_equal_bits(per_node, res, "[rows, F] against [F]")


def test_batches_the_tile_checks_refuse_take_the_layer_route():
    """A bf16 store, a non-finite graph, more than 64 clusters and ``fused=False`` with ``tiles`` set (four steps)."""
    model, ref = _model(30, 2), ig_ref.reference("asym", "t1", steps=4)
    datas = [d.clone() for d in ig_ref.datas("asym")]
    bf16 = GraphStore(pack_graphs(records_from_batch(graph_zoo.batch(datas))), DEV, dtype="bf16")
    datas[3].x[2, 5] = float("nan")
    nonfinite = GraphStore(pack_graphs(records_from_batch(graph_zoo.batch(datas))), DEV)
    finite = [g for g in range(len(datas)) if g != 3]  # noqa: PLR2004
    for tiles in (True, "force"):
        res = attribution.integrated_gradients(model, bf16, target=1, steps=4, tiles=tiles)
        assert res.path == "layers"
        _assert_matches(res, ref, what=f"bf16 store, tiles={tiles}")
        res = attribution.integrated_gradients(model, nonfinite, target=1, steps=4, tiles=tiles)
        assert res.path == "layers"
        _assert_matches(res, ref, graphs=finite, what=f"beside a non-finite graph, tiles={tiles}")
        res = attribution.integrated_gradients(model, _store("asym"), target=1, steps=4, tiles=tiles, fused=False)
        assert res.path == "layers"
        _assert_matches(res, ref, what=f"fused=False, tiles={tiles}")
    store, many = _many_clusters(70, 92)
    assert int(store._sizes[2].max()) > attribution.K0_TILES_MAX  # noqa: SLF001
    res = attribution.integrated_gradients(model, store, target=1, steps=4, tiles=True)
    assert res.path == "layers"
    _assert_matches(res, ig_ref.integrated_gradients(ig_ref.oracle_model(30, 2), many, 1, *ig_ref.nodes(4)), what="K0 = 70")


def test_without_tiles_the_large_graph_stays_on_the_layer_route():
    """``tiles=False`` and the default: as before (four steps, the large graph alone)."""
    ref = ig_ref.integrated_gradients(ig_ref.oracle_model(30, 2), ig_tiles_cases.datas()[2:3], 1, *ig_ref.nodes(4))
    for kw in ({}, {"tiles": False}):
        res = attribution.integrated_gradients(_model(30, 2), _large_store(), indices=[2], target=1, steps=4, **kw)
        assert res.path == "layers"
        _assert_matches(res, ref, what=f"layers {kw}")
    assert attribution.integrated_gradients(_model(30, 2), _large_store(), target=1, steps=4).path == "layers"  # the whole batch, as today
    assert attribution.integrated_gradients(_model(30, 2), _large_store(), indices=[0, 1, 3], target=1, steps=4, tiles=True).path == "fused"
