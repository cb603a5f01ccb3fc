"""TEST INFRASTRUCTURE shared by ``test_width_cases_host.py`` (CPU) and
``test_gpu_widths.py`` (GPU): the whole-model kernels at the node-feature
widths F and output counts OUT on which their code branches, with one fp64
training step of the oracle (``oracle/gnn_ref.py``) per case as the reference.

Graphs: the asymmetric batch of ``graph_zoo`` (eight graphs of 30-70 nodes, 8-16
depth-0 clusters, transposed arrays not aliased) resized to F columns, clusters
kept.  SGAT multiplies its one edge-feature column into every channel, so that
column (a distance of 3-9) is divided by 6: without it the fp32 oracle itself
sits at half the tolerance at (64, 14) and leaves the kernel no budget
(``test_width_cases_host.py`` holds every case to a tenth).  ``k0_over_64`` is
``[asym[0], ring70, asym[1]]`` at F = 8: a 70-node ring with directed chords in
which every node is its own depth-0 cluster, so K0 = 70 sends a graph with
r4(F) <= 32 down the FoutNet / SGAT kernel's branch without the fused front
(GINet's per-graph pass runs the same batch: its depth-0 keys and pooled rows
are sized by K0 too).

Loss: MSE on the stored targets for OUT = 1, else cross entropy with targets
``i % OUT``.  ``loss="mse"`` overrides that for OUT > 1 (test_gpu_multi_output_mse.py):
the stored targets are kept and the loss is the project's multi-output
regression rule, restated from ``engine._layered_step`` and
``engine.loss_scale``: ``((out[:, 0] - y) ** 2).sum() / (B * OUT)``.
"""

from __future__ import annotations

import functools

import numpy as np
import torch
from _util import fixed_dropout

import graph_zoo
from oracle import gnn_ref

# family -> (oracle class, edge features, has dropout)
FAMILIES = {
    "foutnet": (gnn_ref.FoutNet, 3, False),
    "sgat": (gnn_ref.SGAT, 1, False),
    "nocluster": (gnn_ref.GINetNoCluster, 3, True),
    "ginet": (gnn_ref.GINet, 3, True),
}
FOUT_WIDTHS = ((1, 1), (4, 1), (8, 16), (29, 5), (32, 1), (33, 16), (64, 14), (64, 1))
WIDTHS = {
    "foutnet": FOUT_WIDTHS,
    "sgat": FOUT_WIDTHS,
    "nocluster": ((1, 1), (16, 16), (32, 1), (33, 5), (64, 16)),
    "ginet": ((1, 1), (32, 16), (33, 1), (64, 16)),
}
# (F, OUT) of the MSE cases with several outputs (``loss="mse"``): three at the
# batch's own width, 16 (= DR_MAX_OUT) at a width the family already runs
MSE_MULTI = {
    "foutnet": ((30, 3), (33, 16)),
    "sgat": ((30, 3), (33, 16)),
    "nocluster": ((30, 3), (32, 16)),
    "ginet": ((30, 3), (32, 16)),
}
K0_OVER_64 = (8, 16)  # (F, OUT) of the k0_over_64 batch
K0_FAMILIES = ("foutnet", "sgat", "ginet")
SGAT_EDGE_SCALE = 1.0 / 6.0
# parameters whose gradient is exactly zero by construction: the attention's
# softmax runs over a singleton dimension (ginet.py:48-55), so it is identically 1
ZERO_GRADS = ("fc_attention", "fc_edge_attr")


def r4(v):
    return (v + 3) & ~3


def r16(v):
    return (v + 15) & ~15


def image_words(f, out):
    """Words of the FoutNet / SGAT per-graph kernel's flat weight image (six
    registers per thread of 1,024: at most 6,144)."""
    return 32 * f + 3184 + 65 * out


def ring70():
    i = np.arange(70)
    return graph_zoo._graph(np.random.default_rng(5), 70, np.stack([i, (i + 1) % 70], 1), i, i % 5, "ring70", directed=np.stack([i, (i + 7) % 70], 1))  # noqa: SLF001


def datas(family, f, out, batch="asym", loss=None):
    """The graphs of one case, built once per process and left unchanged
    (collate copies of them with ``graph_zoo.batch``)."""
    return _datas(family, f, out, batch, loss)


@functools.lru_cache(maxsize=None)
def _datas(family, f, out, batch, loss):
    fe = FAMILIES[family][1]
    ds = graph_zoo.asymmetric(fe=fe, **graph_zoo.ASYM_BATCH)
    if batch == "k0_over_64":
        assert family in K0_FAMILIES and (f, out) == K0_OVER_64
        ds = [ds[0], ring70(), ds[1]]
    else:
        assert batch == "asym"
    ds = graph_zoo.resized(ds, f, fe)
    for i, d in enumerate(ds):
        if family == "sgat":
            d.edge_attr = d.edge_attr * SGAT_EDGE_SCALE
        if out > 1 and loss != "mse":
            d.y = torch.tensor([float(i % out)])
    return tuple(ds)


def oracle(family, f, out, batch="asym", dtype=torch.float64, loss=None):
    """One training-mode forward + backward of the oracle in ``dtype``:
    ``{"state", "mask", "out", "loss", "grads"}``.  The weights are drawn in
    fp32 under seed 11 (``state``: what the HIP model loads) and the dropout
    mask in fp32 under seed 3 (``torch.rand`` depends on the default dtype),
    whatever ``dtype`` the step then runs in.  Cached per case, dtype and loss
    override."""
    return _oracle(family, f, out, batch, dtype, loss)


@functools.lru_cache(maxsize=None)
def _oracle(family, f, out, batch, dtype, loss):
    assert loss in (None, "mse")
    cls, fe, has_drop = FAMILIES[family]
    ds = datas(family, f, out, batch, loss)
    assert torch.get_default_dtype() == torch.float32
    torch.manual_seed(11)
    model = cls(f, out, fe).train()
    state = {k: v.detach().clone() for k, v in model.state_dict().items()}
    mask = None
    if has_drop:
        mask = (torch.rand(len(ds), 128, generator=torch.Generator().manual_seed(3)) >= 0.4).float()
        model.dropout_fn = fixed_dropout(mask.to(dtype))
    model = model.to(dtype)
    torch.set_default_dtype(dtype)  # oracle/pyg_ops.py and the layers allocate in the default dtype
    try:
        bat = graph_zoo.batch(ds)
        for k in ("x", "edge_attr", "pos", "y"):
            setattr(bat, k, getattr(bat, k).to(dtype))
        y = bat.y.clone()
        res = model(bat)
        if out == 1:
            lval = torch.nn.functional.mse_loss(res.reshape(-1), y)
        elif loss == "mse":  # column 0 alone, 1 / (B * OUT)
            lval = ((res[:, 0] - y) ** 2).sum() / (len(ds) * out)
        else:
            lval = torch.nn.functional.cross_entropy(res, y.long())
        lval.backward()
    finally:
        torch.set_default_dtype(torch.float32)
    assert res.dtype == dtype and all(p.grad.dtype == dtype for p in model.parameters())
    grads = {n: p.grad.detach().numpy().copy() for n, p in model.named_parameters()}
    return {"state": state, "mask": mask, "out": res.detach().numpy().copy(), "loss": float(lval.detach()), "grads": grads}


@functools.lru_cache(maxsize=None)
def packed(family, f, out, batch="asym", loss=None):
    """The case's graphs in the store layout (host side; shared, unchanged)."""
    from deeprank2_amd.store import pack_graphs, records_from_batch  # noqa: PLC0415

    return pack_graphs(records_from_batch(graph_zoo.batch(datas(family, f, out, batch, loss))), require_clusters=family != "nocluster")


def case(family, f, out, batch="asym", loss=None):
    """The inputs and the fp64 reference of one GPU case (cached, shared,
    never modified): ``datas``, ``f``, ``out_dim``, ``loss_kind`` ("mse" /
    "ce"; ``loss`` overrides the choice by ``out``), and ``oracle``'s record."""
    kind = loss or ("mse" if out == 1 else "ce")
    return {"datas": datas(family, f, out, batch, loss), "f": f, "out_dim": out, "loss_kind": kind, **oracle(family, f, out, batch, loss=loss)}


def all_cases():
    """(family, F, OUT, batch) of every case."""
    cs = [(fam, f, out, "asym") for fam, ws in WIDTHS.items() for f, out in ws]
    return cs + [(fam, *K0_OVER_64, "k0_over_64") for fam in K0_FAMILIES]


def is_zero_grad(family, name):
    return family in ("ginet", "nocluster") and any(z in name for z in ZERO_GRADS)


def grad_ntol(family, force_large):
    """``assert_grad_close``'s normwise floor: 1e-6, and 1e-5 on
    ginet_nocluster's tile pipeline (test_gpu_ginet_nocluster.py)."""
    return 1e-5 if family == "nocluster" and force_large else 1e-6


def ratios(got, ref, ntol=1e-6):
    """Per tensor, the largest |got - ref| as a fraction of what the GPU
    comparison allows at that element: outputs rtol = atol = 1e-4, loss 1e-4
    relative, gradients ``assert_grad_close`` (rtol 1e-4, atol
    max(1e-6, ntol max|ref|)).  A ratio above 1 fails that comparison."""

    def worst(a, r, rtol, atol):
        a, r = np.asarray(a, np.float64), np.asarray(r, np.float64)
        return float((np.abs(a - r) / (atol + rtol * np.abs(r))).max())

    res = {"out": worst(got["out"], ref["out"], 1e-4, 1e-4), "loss": abs(got["loss"] - ref["loss"]) / (1e-4 * abs(ref["loss"]))}
    for n, g in ref["grads"].items():
        res[n] = worst(got["grads"][n], g, 1e-4, max(1e-6, ntol * float(np.abs(g).max())))
    return res
