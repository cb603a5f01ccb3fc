"""GINet integrated gradients (``attribution.integrated_gradients`` /
``dr_ginet_integrated_grad_pass``) against the fp64 CPU reference of
``ig_ref.py``, and the properties that hold bit for bit.

Batches: ``graph_zoo.asymmetric`` (A != A^T at node and pooled level, self
loops, a duplicated edge), ``graph_zoo.degenerate`` (N = 1, edgeless graphs, a
hub row, K0 = N = 24, N at and beside 16 / 32 / 64 / 128), and the F = 33
(KPT = 64) and F = 12 normal-feature batches.  Eight Gauss-Legendre nodes
unless a test says otherwise.

Tolerances are the suite's (``ig_ref``'s docstring): outputs rtol = atol =
1e-4; attributions ``_util.assert_grad_close`` per graph; ``attr_sum`` and
``delta`` that element tolerance summed over the graph,
|got - ref| <= 1e-4 sum|attr_ref| + N F max(1e-6, 1e-6 max|attr_ref|)."""

from __future__ import annotations

import numpy as np
import pytest
import torch
from _util import assert_grad_close

import graph_zoo
import ig_ref
from attribution_ref import DEV
from attribution_ref import model as _model
from attribution_ref import store as _store
from deeprank2_amd import _lib, attribution
from deeprank2_amd.fused import LDS_MAX
from deeprank2_amd.store import GraphStore, pack_graphs, records_from_batch
from deeprank2_amd.utils.synthetic import make_dataset
from oracle import data_ref

pytestmark = pytest.mark.gpu


def _baseline(batch, kind, full=False):
    b = ig_ref.baseline_of(batch, kind)
    if b is not None and full:  # the same baseline spelled per node
        b = b.expand(sum(d.x.shape[0] for d in ig_ref.datas(batch)), -1).contiguous()
    return b


def _run(batch, name="t1", kind="zero", steps=8, use_z=True, full=False, **kw):
    out_dim, target = ig_ref.target_of(batch, name)
    store = _store(batch)
    store.use_agg_x = use_z
    key = "seed" if isinstance(target, torch.Tensor) else "target"
    try:
        res = attribution.integrated_gradients(_model(ig_ref.n_feat(batch), out_dim), store, **{key: target}, baseline=_baseline(batch, kind, full), steps=steps, **kw)
        torch.cuda.synchronize()
    finally:
        store.use_agg_x = True
    return res


def _assert_matches(res, ref, graphs=None, what=""):
    off = ref["node_off"]
    graphs = range(len(off) - 1) if graphs is None else graphs
    assert res.attr.shape == ref["attr"].shape and np.array_equal(res.node_off, off)
    attr, attr_sum, delta = res.attr.cpu().numpy(), res.attr_sum.cpu().numpy(), res.delta.cpu().numpy()
    assert attr_sum.dtype == delta.dtype == np.float64
    out, out_b, seed = res.out.cpu().numpy(), res.out_baseline.cpu().numpy(), res.seed.cpu().numpy()
    for g in graphs:
        rows = slice(off[g], off[g + 1])
        np.testing.assert_allclose(out[g], ref["out"][g], **ig_ref.TOL, err_msg=f"{what} out of graph {g}")
        np.testing.assert_allclose(out_b[g], ref["out_baseline"][g], **ig_ref.TOL, err_msg=f"{what} out_baseline of graph {g}")
        np.testing.assert_array_equal(seed[g], ref["seed"][g], err_msg=f"{what} seed of graph {g}")
        assert_grad_close(attr[rows], ref["attr"][rows], err_msg=f"{what} attr of graph {g}")
        np.testing.assert_array_equal(res.graph(g).cpu().numpy(), attr[rows])
        tol = ig_ref.sum_tolerance(ref, g)
        assert abs(attr_sum[g] - ref["attr_sum"][g]) <= tol, (what, g, attr_sum[g], ref["attr_sum"][g], tol)
        assert abs(delta[g] - ref["delta"][g]) <= tol, (what, g, delta[g], ref["delta"][g], tol)
    assert np.array_equal(res.alpha, ig_ref.nodes(res.alpha.size)[0]) and res.alpha.dtype == np.float32


# --------------------------------------------------------------------------
# 1. against the fp64 reference
# --------------------------------------------------------------------------


@pytest.mark.parametrize("groups", [1, 3, 8])  # 3: uneven step ranges (2, 3, 3); 8: one step per workgroup
@pytest.mark.parametrize("name", list(ig_ref.TARGETS))
@pytest.mark.parametrize("batch", ["asym", "deg"])
def test_integrated_gradients_vs_reference(batch, name, groups):
    res = _run(batch, name, groups=groups)
    assert res.path == "fused"
    _assert_matches(res, ig_ref.reference(batch, name), what=f"{batch}/{name}/G{groups}")


@pytest.mark.parametrize("batch", ["f33", "f12"])
def test_integrated_gradients_other_feature_counts(batch):
    """F = 33: the KPT = 64 kernel, 16 chunks per Z row and x_stride 36; F = 12."""
    assert _store(batch).x_stride == {"f33": 36, "f12": 12}[batch]
    res = _run(batch, "t1", groups=3)
    assert res.path == "fused"
    _assert_matches(res, ig_ref.reference(batch, "t1"), what=batch)


def test_default_groups_and_steps():
    res = _run("asym", "t1", steps=32)
    assert res.path == "fused" and res.alpha.size == res.weight.size == 32
    _assert_matches(res, ig_ref.reference("asym", "t1", steps=32), what="defaults")
    assert torch.equal(res.attr, _run("asym", "t1", steps=32, groups=min(attribution.IG_GROUPS_DEFAULT, 32)).attr)


# --------------------------------------------------------------------------
# 2. non-zero baselines
# --------------------------------------------------------------------------


@pytest.mark.parametrize("batch", ["asym", "f33"])
def test_mean_baseline_as_a_vector_and_as_a_tensor(batch):
    vec, full = _run(batch, "t1", "mean", groups=3), _run(batch, "t1", "mean", groups=3, full=True)
    assert vec.path == full.path == "fused"
    ref = ig_ref.reference(batch, "t1", "mean")
    _assert_matches(vec, ref, what=f"{batch} [F] baseline")
    for k in ("attr", "out", "out_baseline", "attr_sum", "delta"):
        assert torch.equal(getattr(vec, k), getattr(full, k)), k
    assert np.abs(ref["out_baseline"] - ig_ref.reference(batch, "t1")["out_baseline"]).max() > 1e-3  # a different point


# --------------------------------------------------------------------------
# 3. the degenerate quadrature is the input-gradient pass
# --------------------------------------------------------------------------


@pytest.mark.parametrize("batch", ["asym", "deg", "f33"])
def test_one_step_at_alpha_one_equals_x_times_input_gradients_bit_for_bit(batch):
    out_dim, seed = ig_ref.target_of(batch, "seed")
    store, model = _store(batch), _model(ig_ref.n_feat(batch), out_dim)
    store.use_agg_x = True
    res = attribution.integrated_gradients(model, store, seed=seed, groups=1, _quadrature=([1.0], [1.0]))
    grad = attribution.input_gradients(model, store, seed=seed)
    assert res.path == grad.path == "fused" and res.alpha.tolist() == res.weight.tolist() == [1.0]
    assert torch.equal(res.attr, store.x[:, : store.n_feat] * grad.dx)
    assert torch.equal(res.out, grad.out)
    assert res.attr.abs().max() > 0


# --------------------------------------------------------------------------
# 4. determinism and layout
# --------------------------------------------------------------------------


@pytest.mark.parametrize(("batch", "kind"), [("asym", "zero"), ("deg", "zero"), ("f33", "mean")])
def test_repeated_calls_are_bit_identical(batch, kind):
    a, b = _run(batch, "seed", kind, groups=3), _run(batch, "seed", kind, groups=3)
    assert a.path == b.path == "fused"
    for k in ("attr", "out", "out_baseline", "attr_sum", "delta"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    assert torch.isfinite(a.attr).all()


def test_graph_alone_equals_its_rows_inside_a_batch():
    store = _store("deg")
    store.use_agg_x = True
    model = _model(30, 2)
    order = [14, 3, 0, 9, 4, 12, 2, 7, 1, 13, 5, 10, 6]  # 13 of the 15 graphs
    seed = torch.randn(len(order), 2, generator=torch.Generator().manual_seed(9))
    inside = attribution.integrated_gradients(model, store, indices=order, seed=seed, steps=8, groups=3)
    for pos in (1, 2, 4, 5, 9):  # star, one node, ring with chords, N = 64, N = 129
        alone = attribution.integrated_gradients(model, store, indices=[order[pos]], seed=seed[pos : pos + 1], steps=8, groups=3)
        assert alone.path == inside.path == "fused"
        assert torch.equal(alone.attr, inside.graph(pos)), order[pos]
        assert torch.equal(alone.out[0], inside.out[pos]) and torch.equal(alone.attr_sum[0], inside.attr_sum[pos])
    assert inside.indices.tolist() == order


@pytest.mark.parametrize(("batch", "kind"), [("deg", "zero"), ("f33", "mean"), ("f12", "zero")])
def test_only_the_requested_rows_are_written(batch, kind):
    store = _store(batch)
    rows, xs, f = int(store.x.shape[0]), store.x_stride, store.n_feat
    buf = torch.full((rows + 64, xs), float("nan"), dtype=torch.float32, device=DEV)
    res = _run(batch, "t1", kind, groups=3, attr_out=buf, batch_size=3)
    assert res.path == "fused" and res.attr.data_ptr() == buf.data_ptr()
    assert torch.isfinite(buf[:rows]).all()
    assert not buf[:rows, f:].any()  # exact zeros in the pad columns
    assert torch.isnan(buf[rows:]).all()
    _assert_matches(res, ig_ref.reference(batch, "t1", kind), what=f"{batch} into a caller's buffer")


def test_rows_without_an_in_edge_are_exactly_zero():
    """dX = A^T dZ: a node no edge points at gets an exact zero row whatever its
    own features and out-edges are."""
    for batch, kind in (("deg", "zero"), ("asym", "mean")):
        res = _run(batch, "seed", kind, groups=3)
        attr = res.attr.cpu().numpy()
        n_zero_rows = 0
        for g, d in enumerate(ig_ref.datas(batch)):
            rows = attr[res.node_off[g] : res.node_off[g + 1]]
            no_in = np.setdiff1d(np.arange(d.x.shape[0]), d.edge_index.numpy()[1])
            assert not rows[no_in].any(), (batch, g)
            n_zero_rows += no_in.size
        assert n_zero_rows > 0 and attr.any()


# --------------------------------------------------------------------------
# 5. the split over workgroups changes the rounding only
# --------------------------------------------------------------------------


@pytest.mark.parametrize("batch", ["asym", "deg"])
def test_one_group_and_four_groups_agree_within_the_tolerance(batch):
    one, four = _run(batch, "seed", groups=1), _run(batch, "seed", groups=4)
    a, b, off = one.attr.cpu().numpy(), four.attr.cpu().numpy(), one.node_off
    for g in range(len(off) - 1):
        assert_grad_close(b[off[g] : off[g + 1]], a[off[g] : off[g + 1]], err_msg=f"G = 4 vs G = 1, graph {g}")
    assert torch.equal(one.out, four.out) and torch.equal(one.out_baseline, four.out_baseline)


# --------------------------------------------------------------------------
# 6. fallbacks (four steps)
# --------------------------------------------------------------------------


@pytest.mark.parametrize("kind", ig_ref.BASELINES)
@pytest.mark.parametrize("how", ["fused_off", "no_agg_x"])
def test_layer_route_agrees_with_the_reference(how, kind):
    res = _run("asym", "pred", kind, steps=4, **({"fused": False} if how == "fused_off" else {"use_z": False}))
    assert res.path == "layers"
    _assert_matches(res, ig_ref.reference("asym", "pred", kind, steps=4), what=f"layers ({how})")


def test_layer_route_takes_a_baseline_as_a_vector_and_as_a_tensor():
    vec, full = _run("asym", "t1", "mean", steps=4, fused=False), _run("asym", "t1", "mean", steps=4, fused=False, full=True)
    assert vec.path == full.path == "layers"
    for k in ("attr", "out", "out_baseline", "attr_sum", "delta"):
        assert torch.equal(getattr(vec, k), getattr(full, k)), k
    assert vec.attr.abs().max() > 0


def test_nonfinite_graph_sends_its_batch_to_the_layer_route():
    datas = [d.clone() for d in ig_ref.datas("asym")]
    datas[3].x[2, 5] = float("nan")
    store = GraphStore(pack_graphs(records_from_batch(graph_zoo.batch(datas))), DEV)
    model = _model(30, 2)
    ref = ig_ref.reference("asym", "t1", steps=4)
    finite = [g for g in range(len(datas)) if g != 3]
    res = attribution.integrated_gradients(model, store, target=1, steps=4)
    assert res.path == "layers"
    _assert_matches(res, ref, graphs=finite, what="beside a non-finite graph")
    split = attribution.integrated_gradients(model, store, target=1, steps=4, batch_size=3)  # [0 1 2] fused, [3 4 5] layers, [6 7] fused
    assert split.path == "mixed"
    _assert_matches(split, ref, graphs=finite, what="split around a non-finite graph")


def test_graph_beyond_one_workgroup_takes_the_layer_route():
    """One graph sized from dr_ginet_integrated_grad_lds_bytes to exceed one
    workgroup's LDS (degree 8; about N = 1 000), beside a small one."""
    q = _lib.load().dr_ginet_integrated_grad_lds_bytes
    n = next(n for n in range(600, 4000, 100) if q(n, 6 * n, 30, 4, 12, 1, 1, 2, 36) > LDS_MAX + 8 * 1024)
    (big,) = make_dataset(1, seed=81, n_lo=n, n_hi=n, mean_degree=8.0, k_lo=4, k_hi=4)
    (small,) = make_dataset(1, seed=82, n_lo=20, n_hi=60, mean_degree=6.0, k_lo=2, k_hi=13)
    datas = [data_ref.synthetic_to_data(g, f"g{j}") for j, g in enumerate([small, big])]
    store = GraphStore(pack_graphs(records_from_batch(graph_zoo.batch(datas))), DEV)
    sizes = store.max_sizes([1])
    assert q(*sizes[:2], 30, *sizes[2:], int(store.packed.transpose_aliased), 2, store.agg_x_stride) > LDS_MAX
    model = _model(30, 2)
    ref = ig_ref.integrated_gradients(ig_ref.oracle_model(30, 2), datas[1:], 1, *ig_ref.nodes(4))
    alone = attribution.integrated_gradients(model, store, indices=[1], target=1, steps=4)
    assert alone.path == "layers"
    _assert_matches(alone, ref, what="the large graph alone")
    assert attribution.integrated_gradients(model, store, indices=[0], target=1, steps=4).path == "fused"
    assert attribution.integrated_gradients(model, store, batch_size=1, target=1, steps=4).path == "mixed"


# --------------------------------------------------------------------------
# 7. the model is left alone
# --------------------------------------------------------------------------


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "layers"])
def test_training_flag_and_parameters_are_untouched(fused):
    store = _store("asym")
    store.use_agg_x = True
    for training in (True, False):
        model = _model(30, 2).train(training)
        before = {n: p.detach().clone() for n, p in model.named_parameters()}
        res = attribution.integrated_gradients(model, store, target="pred", steps=4, fused=fused)
        torch.cuda.synchronize()
        assert res.path == ("fused" if fused else "layers")
        assert model.training is training
        for n, p in model.named_parameters():
            assert torch.equal(p.detach(), before[n]), n
            assert p.grad is None and p.requires_grad, n
