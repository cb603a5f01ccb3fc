"""MSE with more than one output, every family and path, against one **fp64**
training step of the CPU oracle.

The project's rule for a regression loss on a model with OUT > 1 outputs: the
loss reads column 0 of the outputs and takes the factor 1 / (B * OUT)
(``engine._layered_step``, ``engine.loss_scale``; ginet_head.h zeroes
``dout[1..OUT)`` with that comment).  Every other whole-model test picks
``"mse" if out == 1 else "ce"``, so the MSE branch of the general (OUT > 1)
heads had never run: in the FoutNet / SGAT head (fout_fused.hip), the Vanilla
pipeline head (vanilla_fused.hip) and the Vanilla per-graph head
(vanilla_graph.hip) it set ``dout[0]`` and left the logits 1.. where the head
backward multiplies them into ``dh`` and into fc2's rows 1 and up: finite,
wrong gradients, and a fused path that disagreed with the layer path.  GINet
and ginet_nocluster (ginet_head.h) are the control.

Reference (``width_cases.oracle(..., loss="mse")`` / ``vanilla_zoo.oracle(...,
out_dim=)``; test_multi_output_mse_host.py and test_vanilla_zoo_host.py check
them on the CPU): the family's oracle forward, ``((out[:, 0] - y) ** 2).sum()
/ (B * OUT)``, gradients by autograd.  Cases: OUT = 3 on the asymmetric batch
and OUT = 16 (= DR_MAX_OUT) at a width the family already runs, on the
per-graph kernel and the forced tile + tail path (VanillaNetwork: the
per-graph kernel with 1 and 4 workgroups per graph, the chunk-fused and the
untiled pipeline).  Checked: outputs, loss and every gradient under the
family's existing rule; the last linear layer's gradient rows and bias entries
from 1 on ``== 0`` exactly; and the forced layer path (``h.force_layers``) of
the same batch against the fused one under the same tolerance.

On the kernels before the fix (one run, MI355X): see DESIGN.md §5.
"""

from __future__ import annotations

import functools

import numpy as np
import pytest
import torch
import vanilla_zoo as V
import width_cases as W
from _util import assert_grad_close
from test_gpu_vanilla_zoo import _assert_path as _assert_vanilla_path
from test_gpu_widths import MODELS, PATHS, TOL, _assert_path

from deeprank2_amd.engine import FusedTrainStep
from deeprank2_amd.fused import BatchHandle
from deeprank2_amd.neuralnets.gnn import vanilla_gnn
from deeprank2_amd.store import GraphStore

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = [(fam, f, out) for fam, ws in W.MSE_MULTI.items() for f, out in ws]
IDS = lambda c: f"{c[0]}-F{c[1]}-OUT{c[2]}"  # noqa: E731


@functools.lru_cache(maxsize=None)
def _store(family, f, out):
    return GraphStore(W.packed(family, f, out, "asym", "mse"), DEV)


def _train_step(family, f, out, force_layers=False, **knobs):
    """One ``FusedTrainStep.step`` with ``loss="mse"`` from the case's
    parameters (GINets: the case's fixed dropout mask, as
    test_gpu_widths._train_step): outputs, loss and gradients."""
    c = W.case(family, f, out, loss="mse")
    assert c["loss_kind"] == "mse" and c["out_dim"] == out > 1
    h = BatchHandle(_store(family, f, out), np.arange(len(c["datas"])))
    for k, v in knobs.items():
        setattr(h, k, v)
    h.force_layers = force_layers
    model = MODELS[family][1](f, out, W.FAMILIES[family][1])
    model.load_state_dict(c["state"])
    step = FusedTrainStep(model.to(DEV).train(), loss="mse")
    step.acc = False
    assert step.loss_scale(h, h.B) == 1.0 / (h.B * out)
    loss, res = step.step(h, mask=None if c["mask"] is None else c["mask"].to(torch.uint8).to(DEV))
    torch.cuda.synchronize()
    if not force_layers:
        _assert_path(family, h, out, knobs.get("force_large", False), knobs.get("large_halos", True))
    names = MODELS[family][0].PARAM_NAMES
    return {"out": res.cpu().numpy().copy(), "loss": float(loss), "grads": {n: g.cpu().numpy().copy() for n, g in zip(names, step.grads)}}


def _assert_rows_from_1_are_zero(grads, weight="fc2.weight", bias="fc2.bias"):
    w, b = grads[weight], grads[bias]
    assert np.all(w[1:] == 0), f"{weight}: rows 1.. hold up to {np.abs(w[1:]).max():.3g} (row 0: {np.abs(w[0]).max():.3g})"
    assert np.all(b[1:] == 0), f"{bias}: entries 1.. hold up to {np.abs(b[1:]).max():.3g}"
    assert np.any(w[0]) and b[0] != 0


def _assert_close(family, got, ref, ntol, what):
    r = W.ratios(got, ref, ntol=ntol)
    worst = max(r, key=r.get)
    print(f"[mse {what}] worst {worst}: {r[worst]:.3f} of the tolerance; out {r['out']:.3f} loss {r['loss']:.3f}; fc2 rows 1..: {np.abs(got['grads']['fc2.weight'][1:]).max():.3g}")
    assert got["out"].shape == ref["out"].shape
    np.testing.assert_allclose(got["out"], ref["out"], **TOL)
    assert got["loss"] == pytest.approx(ref["loss"], rel=1e-4)
    assert set(got["grads"]) == set(ref["grads"])
    for n, g in ref["grads"].items():
        assert_grad_close(got["grads"][n], g, ntol=ntol, err_msg=n)


@pytest.mark.parametrize("path", ["per_graph", "large"])
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_mse_with_several_outputs_vs_fp64_oracle(c, path):
    """The per-graph kernel and the forced tile + tail path of every family."""
    family, f, out = c
    got = _train_step(family, f, out, **PATHS[path])
    ref = W.case(family, f, out, loss="mse")
    assert not np.any(ref["grads"]["fc2.weight"][1:]) and not np.any(ref["grads"]["fc2.bias"][1:])
    print(f"[mse {IDS(c)} {path}] fc2.weight rows 1..: max {np.abs(got['grads']['fc2.weight'][1:]).max():.3g}, row 0: max {np.abs(got['grads']['fc2.weight'][0]).max():.3g}")
    _assert_rows_from_1_are_zero(got["grads"])
    for n in ref["grads"]:
        if W.is_zero_grad(family, n):
            assert not np.any(got["grads"][n]), f"{n}: expected exact zeros"
    _assert_close(family, got, ref, W.grad_ntol(family, path == "large"), f"{IDS(c)} {path}")


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_layer_path_agrees_with_the_fused_path(c):
    """``h.force_layers``: the layer-level forward with the loss of
    ``engine._layered_step`` and autograd, against the fp64 oracle and against
    the per-graph kernel's step of the same batch, under the same tolerance."""
    family, f, out = c
    ref = W.case(family, f, out, loss="mse")
    layers = _train_step(family, f, out, force_layers=True)
    fused = _train_step(family, f, out, **PATHS["per_graph"])
    ntol = W.grad_ntol(family, False)
    _assert_rows_from_1_are_zero(layers["grads"])
    _assert_close(family, layers, ref, ntol, f"{IDS(c)} layers vs oracle")
    _assert_close(family, fused, layers, ntol, f"{IDS(c)} fused vs layers")


# --------------------------------------------------------------------------
# VanillaNetwork (no layer path: its pipeline is the large-graph path)
# --------------------------------------------------------------------------

VANILLA_PATHS = {
    "per_graph_k1": dict(pipeline=False, vanilla_split=1),
    "per_graph_k4": dict(pipeline=False, vanilla_split=4),
    "chunk": dict(pipeline=True, vanilla_tile_rows=64),
    "untiled": dict(pipeline=True, vanilla_tile_rows=0),
}


@pytest.mark.parametrize("path", list(VANILLA_PATHS))
@pytest.mark.parametrize(("name", "out_dim"), V.MSE_MULTI, ids=[f"{n}-OUT{o}" for n, o in V.MSE_MULTI])
def test_vanilla_mse_with_several_outputs_vs_float64_oracle(name, out_dim, path):
    """vanilla_graph_kernel's head with 1 and 4 workgroups per graph, and the
    pipeline's head kernel behind the chunk-fused and the untiled kernels:
    ``vanilla_zoo.train_step``'s checks, and the last layer's rows 1.. exactly
    zero."""
    f, fe, _ = V.BATCHES[name]
    g64 = V.oracle(name, "mse", "f64", out_dim)[3]
    assert not np.any(g64["_graph_mlp.2.weight"][1:]) and not np.any(g64["_graph_mlp.2.bias"][1:])
    got = {}
    try:
        h = V.train_step(name, "mse", out_dim=out_dim, got=got, **VANILLA_PATHS[path])
    finally:
        if got:
            w = got["grads"]["_graph_mlp.2.weight"]
            print(f"[mse vanilla {name} OUT={out_dim} {path}] _graph_mlp.2.weight rows 1..: max {np.abs(w[1:]).max():.3g}, row 0: max {np.abs(w[0]).max():.3g}")
    _assert_rows_from_1_are_zero(got["grads"], "_graph_mlp.2.weight", "_graph_mlp.2.bias")
    if path.startswith("per_graph"):
        k = VANILLA_PATHS[path]["vanilla_split"]
        assert vanilla_gnn.fused_fits(h, f, fe) and vanilla_gnn.split_k(h, f, fe) == k
        assert h.vanilla_sync_ok() and int(h.vanilla_fused_scratch()[2].abs().sum()) == 0
    else:
        assert not vanilla_gnn.fused_fits(h, f, fe)
        assert _assert_vanilla_path(name, h) == path
