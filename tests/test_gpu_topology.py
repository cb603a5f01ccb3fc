"""The whole-model fused kernels on asymmetric and on degenerate graphs
(``graph_zoo``), against the CPU oracle (``oracle/gnn_ref.py``).

Every other whole-model GPU test feeds doubled (symmetric) edges: the packer
then sets ``transpose_aliased`` and the kernels read ``col`` / ``p1`` for both
directions, so their ``!alias`` carve regions, DMA staging and backward
gathers through ``t_col`` / ``p1t`` never differ from the forward ones.  Here:

* the asymmetric batch (transposed CSR and transposed pooled CSR differ from
  the forward ones on every graph; tests/test_store_topology.py asserts it and
  that a ``p1`` for ``p1t`` mix-up would be far outside these tolerances)
  through GINet, FoutNet, SGAT and ginet_nocluster: the per-graph kernels, the
  forced tile + tail paths, the module autograd path and GINet's accumulating
  pass;
* the degenerate batch (N = 1, graphs without edges, a hub row, every node its
  own depth-0 cluster, N at and beside 16 / 32 / 64 / 128) through the same.

Tolerances are the suite's: outputs rtol = atol = 1e-4, loss 1e-4 relative,
gradients ``_util.assert_grad_close`` (ntol 1e-5 on ginet_nocluster's large
pipeline, as test_gpu_ginet_nocluster.py), Adam against torch.optim.Adam at
rtol 1e-5 / atol 1e-7; the accumulating pass against the per-graph step as in
test_gpu_acc_pass.py."""

from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch
from _util import assert_grad_close, fixed_dropout

import graph_zoo
from deeprank2_amd import _lib
from deeprank2_amd.engine import FusedTrainStep
from deeprank2_amd.fused import LDS_MAX, BatchHandle, Dropout, lds_for
from deeprank2_amd.neuralnets.gnn import foutnet, ginet, ginet_nocluster, sgat
from deeprank2_amd.store import GraphStore, pack_graphs, records_from_batch
from oracle import gnn_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = dict(rtol=1e-4, atol=1e-4)
GRAD_TOL = 1e-5  # accumulating pass vs per-graph step: x max |grad| of the parameter (test_gpu_acc_pass.py)
LOSS_TOL = 1e-6  # relative

# name -> (module, model class, oracle class, edge features, has dropout, plan kind of the large path)
MODELS = {
    "ginet": (ginet, ginet.GINet, gnn_ref.GINet, 3, True, "ginet"),
    "foutnet": (foutnet, foutnet.FoutNet, gnn_ref.FoutNet, 3, False, "fout"),
    "sgat": (sgat, sgat.SGAT, gnn_ref.SGAT, 1, False, "sgat"),
    "nocluster": (ginet_nocluster, ginet_nocluster.GINet, gnn_ref.GINetNoCluster, 3, True, None),
}


@functools.lru_cache(maxsize=None)
def _datas(batch, fe):
    """The graphs of a named batch (shared: collate copies with graph_zoo.batch)."""
    if batch == "asym":
        return tuple(graph_zoo.asymmetric(fe=fe, **graph_zoo.ASYM_BATCH))
    if batch == "deg":
        return tuple(graph_zoo.degenerate(fe=fe))
    if batch == "deg_edges":  # without the two graphs that have no edges
        return tuple(graph_zoo.degenerate(fe=fe, edgeless=False))
    assert batch == "one_node"
    return tuple(graph_zoo.degenerate(fe=fe)[:1])


@functools.lru_cache(maxsize=None)
def _oracle(name, batch, loss="mse"):
    """One training-mode forward + backward of the oracle (fixed dropout mask
    where the model has dropout): (initial state dict, mask, outputs, loss,
    gradients by parameter name).  ``loss``: "mse" on the stored targets
    (1 output) or "ce" over 3 classes (targets i % 3)."""
    _, _, ref_cls, fe, has_drop, _ = MODELS[name]
    datas = _datas(batch, fe)
    out_dim = 1 if loss == "mse" else 3
    torch.manual_seed(11)
    model_o = ref_cls(30, out_dim, fe).train()
    state = {k: v.detach().clone() for k, v in model_o.state_dict().items()}
    mask = None
    if has_drop:
        mask = (torch.rand(len(datas), 128, generator=torch.Generator().manual_seed(3)) >= 0.4).float()
        model_o.dropout_fn = fixed_dropout(mask)
    bat = graph_zoo.batch(datas)
    y = bat.y.clone()
    out = model_o(bat)
    if loss == "mse":
        lval = torch.nn.functional.mse_loss(out.reshape(-1), y)
    else:
        lval = torch.nn.functional.cross_entropy(out, torch.arange(len(datas)) % 3)
    lval.backward()
    grads = {n: p.grad.detach().numpy().copy() for n, p in model_o.named_parameters()}
    return state, mask, out.detach().numpy(), float(lval.detach()), grads


def _model(name, state, out_dim=1):
    _, cls, _, fe, _, _ = MODELS[name]
    m = cls(30, out_dim, fe)
    m.load_state_dict(state)
    return m.to(DEV).train()


def _handle(name, batch, force_large=False):
    fe = MODELS[name][3]
    datas = _datas(batch, fe)
    packed = pack_graphs(records_from_batch(graph_zoo.batch(datas)), require_clusters=name != "nocluster")
    h = BatchHandle(GraphStore(packed, DEV), np.arange(len(datas)))
    h.force_large = force_large
    return h


def _assert_path(name, h, force_large, out_dim=1):
    """The launch took the kernels the test is about."""
    mod, kind = MODELS[name][0], MODELS[name][5]
    assert lds_for(mod.SPEC, h, out_dim) <= LDS_MAX  # small graphs: the large path only when forced
    plan = h._lds.get("nc_plan") if kind is None else h._lds.get(("large", out_dim, False, kind))  # noqa: SLF001
    assert (plan is not None) == force_large


def _is_symmetric(d):
    ei = d.edge_index.numpy()
    n = d.x.shape[0]
    return np.array_equal(np.sort(ei[0] * n + ei[1]), np.sort(ei[1] * n + ei[0]))


def _check_train_step(name, batch, force_large):
    """FusedTrainStep.step on the batch: forward output, in-kernel MSE loss,
    every parameter gradient and the Adam update against the oracle."""
    mod = MODELS[name][0]
    state, mask, out_o, loss_o, grads_o = _oracle(name, batch)
    if name == "foutnet":  # (mean over an empty neighbourhood is NaN: these batches have none that survives the pooling)
        assert np.isfinite(out_o).all() and all(np.isfinite(g).all() for g in grads_o.values())
    model = _model(name, state)
    h = _handle(name, batch, force_large)
    assert h.store.packed.transpose_aliased == all(_is_symmetric(d) for d in _datas(batch, MODELS[name][3]))
    if batch == "asym":
        assert not h.store.packed.transpose_aliased
    step = FusedTrainStep(model)
    step.acc = False
    before = [p.detach().clone() for p in step.params]
    loss, out = step.step(h, mask=None if mask is None else mask.to(torch.uint8).to(DEV))
    torch.cuda.synchronize()
    _assert_path(name, h, force_large)
    np.testing.assert_allclose(out.cpu().numpy(), out_o, **TOL)
    assert float(loss) == pytest.approx(loss_o, rel=1e-4)
    ntol = 1e-5 if (name == "nocluster" and force_large) else 1e-6
    for n, g in zip(mod.PARAM_NAMES, step.grads):
        assert_grad_close(g.cpu().numpy(), grads_o[n], ntol=ntol, err_msg=n)
    # the fused Adam against torch.optim.Adam fed the same (kernel) gradients
    ref = [torch.nn.Parameter(b) for b in before]
    for r, g in zip(ref, step.grads):
        r.grad = g.detach().clone()
    torch.optim.Adam(ref, lr=1e-3, weight_decay=1e-5).step()
    for n, r, p in zip(mod.PARAM_NAMES, ref, step.params):
        np.testing.assert_allclose(p.detach().cpu().numpy(), r.detach().cpu().numpy(), rtol=1e-5, atol=1e-7, err_msg=n)


# --------------------------------------------------------------------------
# asymmetric batch
# --------------------------------------------------------------------------


@pytest.mark.parametrize("force_large", [False, True], ids=["per_graph", "large"])
@pytest.mark.parametrize("name", list(MODELS))
def test_asymmetric_train_step_vs_oracle(name, force_large):
    """Per-graph kernels, and the forced large-graph paths (dr_ginet_large_pass,
    dr_fout_large_pass, dr_sgat_large_pass, dr_ginet_nocluster_large_pass), with
    transposed arrays that differ from the forward ones."""
    _check_train_step(name, "asym", force_large)


@pytest.mark.parametrize("force_large", [False, True], ids=["per_graph", "large"])
@pytest.mark.parametrize("name", ["ginet", "foutnet"])
def test_asymmetric_module_autograd_vs_oracle(name, force_large):
    """``model(batch)`` -> cross-entropy over 3 classes -> ``backward()``:
    FusedFn's backward pass with an upstream ``dout``."""
    state, mask, out_o, loss_o, grads_o = _oracle(name, "asym", "ce")
    if name == "foutnet":
        assert np.isfinite(out_o).all() and all(np.isfinite(g).all() for g in grads_o.values())
    model = _model(name, state, out_dim=3)
    h = _handle(name, "asym", force_large)
    assert not h.store.packed.transpose_aliased
    batch = SimpleNamespace(_dr_handle=h)
    out = model(batch) if mask is None else model(batch, dropout_mask=mask.to(torch.uint8))
    loss = torch.nn.functional.cross_entropy(out, (torch.arange(h.B) % 3).to(DEV))
    loss.backward()
    _assert_path(name, h, force_large, out_dim=3)
    np.testing.assert_allclose(out.detach().cpu().numpy(), out_o, **TOL)
    assert float(loss.detach()) == pytest.approx(loss_o, rel=1e-4)
    for n, p in model.named_parameters():
        assert_grad_close(p.grad.cpu().numpy(), grads_o[n], err_msg=n)


def _pass_outputs(name, h, params, configs):
    """(out, slab, head, per-graph loss) of one FORWARD|BACKWARD graph pass per
    handle configuration (CE over 2 classes; GINet: hash dropout)."""
    mod = MODELS[name][0]
    b = h.B
    h.store.set_targets(np.arange(b) % 2)
    res = []
    for cfg in configs:
        for k, v in cfg.items():
            setattr(h, k, v)
        h._lds.clear()  # noqa: SLF001  (plans are cached per handle: rebuilt for this configuration)
        out = torch.empty(b, 2, device=DEV)
        slab = torch.empty(b * mod.SPEC.slab_stride(30), device=DEV)
        head = torch.zeros(b * mod.SPEC.head_stride(2), device=DEV)
        lpg = torch.empty(b, device=DEV)
        drop = {"dropout": Dropout(0.4, seed=7, offset=3)} if name == "ginet" else {}
        mod.graph_pass(h, params, 2, _lib.DR_PASS_FORWARD | _lib.DR_PASS_BACKWARD, loss_kind=_lib.DR_LOSS_CE, loss_scale=1 / b, out=out, loss_per_graph=lpg, slab=slab, head=head, **drop)
        torch.cuda.synchronize()
        _assert_path(name, h, cfg["force_large"], out_dim=2)
        res.append((out.cpu(), slab.cpu(), head.cpu(), lpg.cpu()))
    return res


GINET_LARGE = [dict(force_large=True, large_halos=hl, large_atomic_max=am) for hl in (True, False) for am in (True, False)]
FOUT_LARGE = [dict(force_large=True, large_halos=hl) for hl in (True, False)]


@pytest.mark.parametrize(("name", "batch"), [("ginet", "asym"), ("foutnet", "asym"), ("sgat", "asym"), ("ginet", "deg"), ("foutnet", "deg_edges"), ("sgat", "deg")])
def test_large_path_bit_identical_to_single_workgroup_kernel(name, batch):
    """test_gpu_large.py's / test_gpu_fout_large.py's assertion, which those make
    on symmetric graphs only: outputs, slab, head and per-graph loss of the tile
    + tail path equal the single-workgroup kernel's bit for bit (GINet: with and
    without halos, with and without the atomic max)."""
    h = _handle(name, batch)
    assert not h.store.packed.transpose_aliased  # (the degenerate batch too: its ring has directed chords)
    torch.manual_seed(5)
    model = MODELS[name][1](30, 2, MODELS[name][3]).to(DEV)
    base = dict(force_large=False, large_halos=True, large_atomic_max=True)
    res = _pass_outputs(name, h, model.ordered_params(), [base, *(GINET_LARGE if name == "ginet" else FOUT_LARGE)])
    assert all(torch.isfinite(t).all() for t in res[0])
    for k, other in enumerate(res[1:]):
        for what, x, y in zip(("out", "slab", "head", "loss"), res[0], other):
            assert torch.equal(x, y), f"configuration {k}: {what}"


def _acc_pair(groups):
    torch.manual_seed(5)
    m1 = ginet.GINet(30, 1, 3).to(DEV).train()
    m2 = ginet.GINet(30, 1, 3).to(DEV).train()
    m2.load_state_dict(m1.state_dict())
    m2._drop_seed = m1._drop_seed = 777  # noqa: SLF001
    acc, per = FusedTrainStep(m1), FusedTrainStep(m2)
    acc.acc, acc.acc_groups = True, groups
    per.acc = False
    return acc, per


def _check_acc_pass(batch, groups):
    """dr_ginet_acc_pass (both prefetch settings) against the per-graph step."""
    h = _handle("ginet", batch)
    _, per = _acc_pair(groups)
    lp, op = per.step(h)
    torch.cuda.synchronize()
    lp, op = lp.clone(), op.clone()
    runs = []
    for prefetch in (True, False):
        acc, _ = _acc_pair(groups)
        acc.acc_prefetch = prefetch
        assert acc._acc_rows(h) == groups and per._acc_rows(h) == 0  # noqa: SLF001
        la, oa = acc.step(h)
        torch.cuda.synchronize()
        assert torch.equal(oa, op), "forward outputs"
        assert abs(float(la) - float(lp)) <= LOSS_TOL * abs(float(lp)), (float(la), float(lp))
        for n, ga, gp in zip(ginet.PARAM_NAMES, acc.grads, per.grads):
            scale = float(gp.abs().max())
            if scale == 0.0:
                assert torch.equal(ga, gp), f"{n} (exact zeros)"
                continue
            err = float((ga.double() - gp.double()).abs().max())
            assert err <= GRAD_TOL * scale, f"prefetch={prefetch} {n}: max|diff| {err:.3g} vs max|grad| {scale:.3g}"
        runs.append((acc.acc_lds(h), [t.clone() for t in acc._state_tensors()]))  # noqa: SLF001
    assert runs[0][0] != runs[1][0], "the prefetch layout must be the one taken"
    for k, (a, b) in enumerate(zip(runs[0][1], runs[1][1])):
        assert torch.equal(a, b), f"prefetch on / off: state tensor {k}"


def test_asymmetric_acc_pass_matches_per_graph_step():
    """8 asymmetric graphs over 2 workgroups: several graphs per workgroup, so
    the prefetch layout stages graph k + 1's ``p1t`` arrays under graph k."""
    _check_acc_pass("asym", 2)


# --------------------------------------------------------------------------
# degenerate batch
# --------------------------------------------------------------------------


@pytest.mark.parametrize("force_large", [False, True], ids=["per_graph", "large"])
@pytest.mark.parametrize(("name", "batch"), [("ginet", "deg"), ("sgat", "deg"), ("nocluster", "deg"), ("foutnet", "deg_edges")])
def test_degenerate_train_step_vs_oracle(name, batch, force_large):
    """N = 1, graphs without edges (not FoutNet: NaN, below), a hub row, K0 = N,
    N at and beside the 16 / 32 / 64 / 128 tile boundaries, in one batch."""
    _check_train_step(name, batch, force_large)


@pytest.mark.parametrize("force_large", [False, True], ids=["per_graph", "large"])
def test_degenerate_foutnet_nan_forward_matches_oracle(force_large):
    """FoutLayer's mean over an empty neighbourhood is NaN (foutnet.py:58): the
    oracle's prediction is NaN exactly for the graphs without edges, and so is
    the kernels'; the other graphs of the same launch are unaffected."""
    datas = _datas("deg", 3)
    torch.manual_seed(11)
    model_o = gnn_ref.FoutNet(30, 1).eval()
    with torch.no_grad():
        out_o = model_o(graph_zoo.batch(datas)).numpy()
    assert np.flatnonzero(np.isnan(out_o).any(axis=1)).tolist() == list(graph_zoo.EDGELESS)
    model = _model("foutnet", model_o.state_dict()).eval()
    h = _handle("foutnet", "deg", force_large)
    with torch.no_grad():
        out = model(SimpleNamespace(_dr_handle=h)).cpu().numpy()
    _assert_path("foutnet", h, force_large)
    np.testing.assert_array_equal(np.isnan(out), np.isnan(out_o))
    np.testing.assert_allclose(out, out_o, equal_nan=True, **TOL)


@pytest.mark.parametrize(("name", "force_large"), [("ginet", False), ("ginet", True), ("nocluster", False)], ids=["ginet-per_graph", "ginet-large", "nocluster-per_graph"])
def test_single_node_graph_alone_vs_oracle(name, force_large):
    """A batch of one graph of one node and no edges (a B = 1 launch).  GINet's
    tile path then has no halo anywhere and gathers per edge; ginet_nocluster's
    tile pipeline refuses such a batch (tests/test_store_topology.py)."""
    _check_train_step(name, "one_node", force_large)


def test_degenerate_acc_pass_matches_per_graph_step():
    """One workgroup runs the whole degenerate batch (acc_groups = 1)."""
    _check_acc_pass("deg", 1)
