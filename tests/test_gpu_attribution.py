"""GINet input gradients (``attribution.input_gradients`` /
``dr_ginet_input_grad_pass``) against the CPU oracle, and the properties that
hold bit for bit.

The reference is ``oracle/gnn_ref.GINet(...).eval()`` with ``x`` requiring
grad and ``torch.autograd.grad((out * seed).sum(), x)`` (attribution_ref.py
says how the batch is handed to it).  Batches: ``graph_zoo.asymmetric`` (A !=
A^T at node and pooled level, self loops, a duplicated edge, 8-16 clusters:
both dP1 paths) and ``graph_zoo.degenerate`` (N = 1, edgeless graphs, a hub
row, directed chords, K0 = N = 24, N at and beside 16 / 32 / 64 / 128).

Tolerances are the suite's: outputs rtol = atol = 1e-4; gradients
``_util.assert_grad_close`` (rtol 1e-4, floor 1e-6 max|ref|), per graph."""

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
from deeprank2_amd.fused import LDS_MAX, BatchHandle
from deeprank2_amd.store import GraphStore, pack_graphs, records_from_batch
from deeprank2_amd.utils.synthetic import make_dataset
from oracle import data_ref

pytestmark = pytest.mark.gpu
TOL = dict(rtol=1e-4, atol=1e-4)


@functools.lru_cache(maxsize=None)
def _oracle(batch, name):
    """(out, dx, seed, node_off) of the oracle on a named batch and target (computed once)."""
    out_dim, target = attribution_ref.target_of(batch, name)
    return attribution_ref.oracle_input_grad(attribution_ref.oracle_model(attribution_ref.n_feat(batch), out_dim), list(attribution_ref.datas(batch)), target)


def _run(batch, name, use_z=True, **kw):
    out_dim, target = attribution_ref.target_of(batch, name)
    store = _store(batch)
    store.use_agg_x = use_z
    key = "seed" if isinstance(target, torch.Tensor) else "target"
    try:
        res = attribution.input_gradients(_model(attribution_ref.n_feat(batch), out_dim), store, **{key: target}, **kw)
        torch.cuda.synchronize()
    finally:
        store.use_agg_x = True
    return res


def _assert_matches_oracle(res, ref, graphs=None, what=""):
    out_o, dx_o, seed_o, off = ref
    graphs = range(len(off) - 1) if graphs is None else graphs
    assert res.dx.shape == dx_o.shape and np.array_equal(res.node_off, off)
    out, dx, seed = res.out.cpu().numpy(), res.dx.cpu().numpy(), res.seed.cpu().numpy()
    for g in graphs:
        np.testing.assert_allclose(out[g], out_o[g], **TOL, err_msg=f"{what} out of graph {g}")
        np.testing.assert_array_equal(seed[g], seed_o[g], err_msg=f"{what} seed of graph {g}")
        assert_grad_close(dx[off[g] : off[g + 1]], dx_o[off[g] : off[g + 1]], err_msg=f"{what} dx of graph {g}")
        np.testing.assert_array_equal(res.graph(g).cpu().numpy(), dx[off[g] : off[g + 1]])


# --------------------------------------------------------------------------
# 1. against the oracle
# --------------------------------------------------------------------------


@pytest.mark.parametrize("use_z", [True, False], ids=["z", "gather"])
@pytest.mark.parametrize("name", list(attribution_ref.TARGETS))
@pytest.mark.parametrize("batch", ["asym", "deg"])
def test_input_gradients_vs_oracle(batch, name, use_z):
    res = _run(batch, name, use_z)
    assert res.path == "fused"
    _assert_matches_oracle(res, _oracle(batch, name), what=f"{batch}/{name}")


@pytest.mark.parametrize("use_z", [True, False], ids=["z", "gather"])
@pytest.mark.parametrize("batch", ["f33", "f12"])
def test_input_gradients_other_feature_counts(batch, use_z):
    """F = 33: the KPT = 64 kernels and x_stride 36 (nine 16-byte chunks per
    row: the ninth goes round the gather's eight lanes again); F = 12."""
    assert _store(batch).x_stride == {"f33": 36, "f12": 12}[batch]
    res = _run(batch, "seed", use_z)
    assert res.path == "fused"
    _assert_matches_oracle(res, _oracle(batch, "seed"), what=batch)


# --------------------------------------------------------------------------
# 2. exact invariants
# --------------------------------------------------------------------------


@pytest.mark.parametrize("batch", ["asym", "deg", "f33"])
def test_z_and_gather_forms_and_repeated_calls_are_bit_identical(batch):
    a, b, c = _run(batch, "seed", True), _run(batch, "seed", True), _run(batch, "seed", False)
    assert a.path == b.path == c.path == "fused"
    assert torch.equal(a.dx, b.dx) and torch.equal(a.out, b.out)
    assert torch.equal(a.dx, c.dx) and torch.equal(a.out, c.out)
    assert torch.isfinite(a.dx).all()


def test_graph_alone_equals_its_rows_inside_a_batch():
    store = _store("deg")
    store.use_agg_x = True
    model = _model(30, 2)
    order = [14, 3, 0, 9, 4, 12, 2, 7, 1, 13, 5, 10, 6]  # 13 of the 15 graphs
    seed = torch.randn(len(order), 2, generator=torch.Generator().manual_seed(9))
    inside = attribution.input_gradients(model, store, indices=order, seed=seed)
    for pos in (1, 2, 4, 5, 9):  # star, one node, ring with chords, N = 64, N = 129
        alone = attribution.input_gradients(model, store, indices=[order[pos]], seed=seed[pos : pos + 1])
        assert alone.path == inside.path == "fused"
        assert torch.equal(alone.dx, inside.graph(pos)), order[pos]
        assert torch.equal(alone.out[0], inside.out[pos])
    assert inside.indices.tolist() == order


def test_out_equals_the_eval_forward():
    for batch, out_dim in (("asym", 1), ("deg", 2)):
        store = _store(batch)
        store.use_agg_x = True
        model = _model(30, out_dim)
        res = attribution.input_gradients(model, store, target=0)
        h = BatchHandle(store, np.arange(store.n_graphs))
        with torch.no_grad():
            fwd = model.eval()(type("B", (), {"_dr_handle": h})())
        assert torch.equal(res.out, fwd)


def test_gradient_is_linear_in_the_seed_exactly():
    out_dim, seed = attribution_ref.target_of("asym", "seed")
    store = _store("asym")
    store.use_agg_x = True
    model = _model(30, out_dim)
    one = attribution.input_gradients(model, store, seed=seed)
    two = attribution.input_gradients(model, store, seed=2.0 * seed)
    assert torch.equal(two.dx, 2.0 * one.dx) and torch.equal(two.out, one.out)
    assert one.dx.abs().max() > 0


@pytest.mark.parametrize("use_z", [True, False], ids=["z", "gather"])
def test_rows_without_an_in_edge_are_exactly_zero(use_z):
    """dX = A^T dZ: node j collects dZ over the edges with edge_index[1] = j.
    The one-node graph, the edgeless graphs and every node no edge points at
    get exact zeros; on the asymmetric batch many such nodes have out-edges, so
    a kernel gathering over the forward CSR gives them non-zero rows."""
    for batch in ("deg", "asym"):
        res = _run(batch, "seed", use_z)
        dx = res.dx.cpu().numpy()
        n_zero_rows = n_with_out_edges = 0
        for g, d in enumerate(attribution_ref.datas(batch)):
            rows = dx[res.node_off[g] : res.node_off[g + 1]]
            ei = d.edge_index.numpy()
            no_in = np.setdiff1d(np.arange(d.x.shape[0]), ei[1])
            assert not rows[no_in].any(), (batch, g)
            n_zero_rows += no_in.size
            n_with_out_edges += np.intersect1d(no_in, ei[0]).size
            if batch == "deg" and g in (0, *graph_zoo.EDGELESS):
                assert no_in.size == d.x.shape[0] and not rows.any()
        assert n_zero_rows > 0
        if batch == "asym":
            assert n_with_out_edges > 0
        assert dx.any()


# --------------------------------------------------------------------------
# 3. bounds
# --------------------------------------------------------------------------


@pytest.mark.parametrize("batch", ["deg", "f33", "f12"])
@pytest.mark.parametrize("use_z", [True, False], ids=["z", "gather"])
def test_only_the_requested_rows_are_written(batch, use_z):
    store = _store(batch)
    rows, xs, f = int(store.x.shape[0]), store.x_stride, store.n_feat
    buf = torch.full((rows + 64, xs), float("nan"), dtype=torch.float32, device=DEV)
    res = _run(batch, "seed", use_z, dx_out=buf, batch_size=3)
    assert res.path == "fused" and res.dx.data_ptr() == buf.data_ptr()
    assert torch.isfinite(buf[:rows]).all()
    assert not buf[:rows, f:].any()  # exact zeros in the pad columns
    assert torch.isnan(buf[rows:]).all()
    _assert_matches_oracle(res, _oracle(batch, "seed"), what=f"{batch} into a caller's buffer")


# --------------------------------------------------------------------------
# 4. fallback
# --------------------------------------------------------------------------


@pytest.mark.parametrize("batch", ["asym", "deg"])
def test_layer_route_agrees_with_the_fused_pass_and_the_oracle(batch):
    layers, fused = _run(batch, "pred", fused=False), _run(batch, "pred")
    assert layers.path == "layers" and fused.path == "fused"
    ref = _oracle(batch, "pred")
    _assert_matches_oracle(layers, ref, what=f"{batch} layers")
    off, a, b = ref[3], layers.dx.cpu().numpy(), fused.dx.cpu().numpy()
    for g in range(len(off) - 1):
        assert_grad_close(a[off[g] : off[g + 1]], b[off[g] : off[g + 1]], err_msg=f"layers vs fused, graph {g}")
    np.testing.assert_allclose(layers.out.cpu().numpy(), fused.out.cpu().numpy(), **TOL)


@functools.lru_cache(maxsize=None)
def _with_large():
    """Three small graphs and one sized from dr_ginet_input_grad_lds_bytes to
    exceed one workgroup's LDS in both forms (degree 8; about N = 1 200)."""
    q = _lib.load().dr_ginet_input_grad_lds_bytes
    # (sized with 6 N edges, fewer than the generator draws at this degree: the test asserts the real sizes)
    n = next(n for n in range(800, 4000, 100) if min(q(n, 6 * n, 30, 4, 12, 1, 1, 2, 0), q(n, 6 * n, 30, 4, 12, 1, 1, 2, 36)) > LDS_MAX + 8 * 1024)
    (big,) = make_dataset(1, seed=81, n_lo=n, n_hi=n, mean_degree=8.0, k_lo=4, k_hi=4)
    small = make_dataset(3, seed=82, n_lo=20, n_hi=60, mean_degree=6.0, k_lo=2, k_hi=13)
    datas = [data_ref.synthetic_to_data(g, f"g{j}") for j, g in enumerate([small[0], small[1], big, small[2]])]
    torch.manual_seed(11)
    ref = attribution_ref.oracle_input_grad(attribution_ref.oracle_model(30, 2), datas, 1)
    return GraphStore(pack_graphs(records_from_batch(graph_zoo.batch(datas))), DEV), ref


def test_graph_beyond_one_workgroup_takes_the_layer_route():
    store, ref = _with_large()
    q = _lib.load().dr_ginet_input_grad_lds_bytes
    alias = int(store.packed.transpose_aliased)
    sizes = store.max_sizes([2])
    for zs in (0, store.agg_x_stride):
        assert q(*sizes[:2], 30, *sizes[2:], alias, 2, zs) > LDS_MAX
    model = _model(30, 2)
    alone = attribution.input_gradients(model, store, indices=[2], target=1)
    assert alone.path == "layers"
    off = ref[3]
    assert_grad_close(alone.dx.cpu().numpy(), ref[1][off[2] : off[3]], err_msg="the large graph alone")
    np.testing.assert_allclose(alone.out.cpu().numpy()[0], ref[0][2], **TOL)
    mixed = attribution.input_gradients(model, store, batch_size=2, target=1)  # [small, small] fused, [large, small] layers
    assert mixed.path == "mixed"
    _assert_matches_oracle(mixed, ref, what="mixed")
    assert attribution.input_gradients(model, store, indices=[0, 1, 3], target=1).path == "fused"


def test_nonfinite_graph_sends_its_batch_to_the_layer_route():
    datas = [d.clone() for d in attribution_ref.datas("asym")]
    datas[3].x[2, 5] = float("nan")
    store = GraphStore(pack_graphs(records_from_batch(graph_zoo.batch(datas))), DEV)
    assert store.packed.nonfinite.tolist() == [g == 3 for g in range(len(datas))]
    model = _model(30, 2)
    res = attribution.input_gradients(model, store, target=1)
    assert res.path == "layers"
    finite = [g for g in range(len(datas)) if g != 3]
    _assert_matches_oracle(res, _oracle("asym", "t1"), graphs=finite, what="beside a non-finite graph")
    split = attribution.input_gradients(model, store, target=1, batch_size=3)  # [0 1 2] fused, [3 4 5] layers, [6 7] fused
    assert split.path == "mixed"
    _assert_matches_oracle(split, _oracle("asym", "t1"), graphs=finite, what="split around a non-finite graph")


@pytest.mark.parametrize("api", ["input_gradients", "integrated_gradients"])
def test_refusals_that_need_the_store(api):
    """What both calls refuse once they hold the store, before any launch: a
    seed, a model or a caller's buffer that does not fit the request, and for
    integrated gradients a per-node baseline that does not."""
    fn, buf_kw = getattr(attribution, api), {"input_gradients": "dx_out", "integrated_gradients": "attr_out"}[api]
    store, model = _store("asym"), _model(30, 2)
    n, rows, xs, f = store.n_graphs, int(store.x.shape[0]), store.x_stride, store.n_feat
    with pytest.raises(ValueError, match="seed must be"):
        fn(model, store, seed=torch.ones(n + 1, 2))
    with pytest.raises(ValueError, match="node features"):
        fn(_model(33, 2), store, target=1)

    def buf(r=rows, c=xs, dtype=torch.float32):
        return torch.zeros(r, c, dtype=dtype, device=DEV)

    for b in (buf(dtype=torch.float64), buf(c=xs + 4), buf(r=rows - 1), buf(c=2 * xs)[:, :xs]):  # fp64, second dimension, too few rows, not contiguous
        with pytest.raises(ValueError, match=f"{buf_kw} must be"):
            fn(model, store, target=1, **{buf_kw: b})
    if api == "integrated_gradients":
        with pytest.raises(ValueError, match="baseline must be"):
            fn(model, store, target=1, baseline=torch.zeros(rows - 1, f))
        twice = [0, 1, 0]
        with pytest.raises(ValueError, match="named once"):
            fn(model, store, indices=twice, target=1, baseline=torch.zeros(int(store._sizes[0][twice].sum()), f))  # noqa: SLF001


# --------------------------------------------------------------------------
# 5. scores
# --------------------------------------------------------------------------


def test_node_scores_and_top_nodes_against_numpy():
    res = _run("asym", "t1")
    store = _store("asym")
    dx = res.dx.cpu().numpy().astype(np.float64)
    x = np.concatenate([d.x.numpy() for d in attribution_ref.datas("asym")]).astype(np.float64)
    want = {"l2": np.sqrt((dx * dx).sum(1)), "l1": np.abs(dx).sum(1), "grad_x_input": (x * dx).sum(1)}
    for kind, w in want.items():
        s = attribution.node_scores(res, store, kind)
        assert s.is_cuda and s.shape == (dx.shape[0],)
        np.testing.assert_allclose(s.cpu().numpy(), w, rtol=1e-5, atol=1e-9, err_msg=kind)
        for i in (0, 5):
            sh = s.cpu().numpy()[res.node_off[i] : res.node_off[i + 1]]
            top = attribution.top_nodes(res, s, i, 4)
            assert top.dtype == np.int64 and top.tolist() == np.argsort(-sh, kind="stable")[:4].tolist()
            assert len(set(top.tolist())) == 4 and sh[top[0]] == sh.max()
    assert (want["grad_x_input"] < 0).any() and (want["grad_x_input"] > 0).any()  # signed
    assert attribution.top_nodes(res, attribution.node_scores(res, store, "l2"), 1, 10_000).size == res.graph(1).shape[0]
    with pytest.raises(ValueError):
        attribution.node_scores(res, store, "saliency")
    # a reordered request scores the rows of the graphs it names
    sub = attribution.input_gradients(_model(30, 2), store, indices=[5, 0], target=1)
    s = attribution.node_scores(sub, store, "grad_x_input").cpu().numpy()
    off = res.node_off
    np.testing.assert_allclose(s, np.concatenate([want["grad_x_input"][off[5] : off[6]], want["grad_x_input"][off[0] : off[1]]]), rtol=1e-5, atol=1e-9)


# --------------------------------------------------------------------------
# 6. the model is left alone
# --------------------------------------------------------------------------


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "layers"])
def test_training_flag_and_parameters_are_untouched(fused):
    store = _store("asym")
    store.use_agg_x = True
    for training in (True, False):
        model = _model(30, 2).train(training)
        before = {n: p.detach().clone() for n, p in model.named_parameters()}
        res = attribution.input_gradients(model, store, target="pred", fused=fused)
        torch.cuda.synchronize()
        assert res.path == ("fused" if fused else "layers")
        assert model.training is training
        for n, p in model.named_parameters():
            assert torch.equal(p.detach(), before[n]), n
            assert p.grad is None, n
