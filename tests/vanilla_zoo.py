"""TEST INFRASTRUCTURE: the VanillaNetwork batches of ``graph_zoo`` with what
the host test (test_vanilla_zoo_host.py) and the GPU test
(test_gpu_vanilla_zoo.py) both need of them: the packed arrays, the pipeline's
tile plan built on the CPU, the host carve sizes with the dispatch rule of
``chunk_fused()`` restated, the oracle in float64 and float32, the tolerance
rule, one training step on the GPU held to them (``train_step``, shared with
test_gpu_vanilla_per_graph_widths.py and test_gpu_multi_output_mse.py), and a
float64 restatement of the network on the packed and planned
arrays (the form the kernels compute, so that a ``col`` for ``t_col`` mix-up
can be put into it).
"""

from __future__ import annotations

import ctypes
import functools

import numpy as np
import torch

import graph_zoo
from deeprank2_amd import _lib
from deeprank2_amd.fused import LDS_MAX, BatchHandle, vanilla_tile_plan
from deeprank2_amd.neuralnets.gnn.vanilla_gnn import PARAM_NAMES
from deeprank2_amd.store import GraphStore, pack_graphs, records_from_batch
from oracle import gnn_ref

CHUNK = 64
CHUNK_F = (12, 29, 32)  # widths on the chunk-fused path ...
CHUNK_FE = (0, 1, 4)
UNFUSED_WIDTHS = ((40, 3), (64, 8), (30, 5))  # ... and beyond it (F > 32 or Fe > 4)
# Widths run on the per-graph kernel alone (vanilla_graph_kernel<FE>,
# test_gpu_vanilla_per_graph_widths.py), outside CHUNK_F x CHUNK_FE: F = 1 (every
# min(.., M - 1) / min(.., Nn - 1) clamp of its GEMMs at 0), F = 4 (x_stride 4),
# F = 15 | 16 (F + 33 = 48 | 49: three | four column tiles of the weight-gradient
# GEMMs; at 16 the upper half of the packed row-pass block is all zero), F = 17
# (its first live row, two row tiles, x_stride 20), F = 31 (F + 33 = 64) and
# F = 32 (five column tiles, no pad column), over every FE instantiation.
PER_GRAPH_ONLY = ((1, 0), (1, 3), (4, 2), (15, 1), (16, 4), (17, 2), (31, 3), (32, 2))
PER_GRAPH_WIDTHS = tuple((f, fe) for f in CHUNK_F for fe in CHUNK_FE) + PER_GRAPH_ONLY
# Seed of the oracle's weights where 11, every other batch's, leaves a narrow
# model dead: at (1, 3) the one node channel's ReLU is off on every node, so
# all eight layer gradients are exactly zero, and at (4, 2) one channel of four
# is live.  The first seeds after 11 with every node channel of layer 2 live
# (test_vanilla_zoo_host.py holds every width to a live gradient per parameter).
SEEDS = {"w1_3": 30, "w4_2": 13}
# Beyond one output and three classes: cross entropy over 16 (= DR_MAX_OUT)
# classes, and (name, out_dim) of the MSE cases with several outputs
CE16 = ("w12_0", "w32_4")
MSE_MULTI = (("asym", 3), ("w12_0", 16))

# name -> (F, Fe, builder of the graphs)
BATCHES = {
    "asym": (30, 3, lambda: graph_zoo.without_clusters(graph_zoo.asymmetric(**graph_zoo.ASYM_BATCH))),
    "deg": (30, 3, lambda: graph_zoo.without_clusters(graph_zoo.degenerate())),
    # the degenerate batch at F = 17, Fe = 2, for the per-graph kernel (its one- and two-node graphs leave siblings of a split without a row)
    "deg17_2": (17, 2, lambda: graph_zoo.without_clusters(graph_zoo.resized(graph_zoo.degenerate(fe=2), 17, 2))),
    "dense3": (30, 3, lambda: graph_zoo.between_small(graph_zoo.dense_tiles(3), 3)),
    "dense4": (30, 4, lambda: graph_zoo.between_small(graph_zoo.dense_tiles(4), 4)),
    "hub_tiled": (30, 3, lambda: graph_zoo.between_small(graph_zoo.hub(graph_zoo.HUB_TILED, y=HUB_Y[0]))),
    "hub_untiled": (30, 3, lambda: graph_zoo.between_small(graph_zoo.hub(graph_zoo.HUB_UNTILED, y=HUB_Y[1]))),
}
# The hub graphs' MSE targets, within 0.1 of what the seeded model predicts for
# them.  A hub row of 1,000 edges is otherwise nearly all of the batch's layer-1
# edge-MLP gradient, which the float32 oracle forms by adding 1,000 equal
# addends per channel one after the other: that alone deviates from float64 by
# 1e-5 of the largest entry, the ceiling of ``grad_atol``.  With the hub graph
# a fifth of the gradient the oracle stays well inside it, and the hub path
# is still checked to the same relative precision (test_vanilla_zoo_host.py
# asserts both).
HUB_Y = (-1.0, -0.8)
for _f, _fe in [(f, fe) for f in CHUNK_F for fe in CHUNK_FE] + list(UNFUSED_WIDTHS) + list(PER_GRAPH_ONLY):
    BATCHES[f"w{_f}_{_fe}"] = (_f, _fe, functools.partial(graph_zoo.widths, _f, _fe))
HARD = {"dense3": 2, "dense4": 2, "hub_tiled": 2, "hub_untiled": 2}  # position of the hard graph (between_small)
WIDTH_BATCHES = tuple(n for n in BATCHES if n.startswith("w"))
# the losses each batch is run with on the GPU (the host test checks the float32 oracle on the same)
LOSSES = {**{n: ("mse",) for n in BATCHES}, "asym": ("mse", "ce"), "deg": ("mse", "ce"), "dense3": ("mse", "ce")}
# 64-row tiles of each batch: (n_tiles, halo_max, tile_edges_max, tile_tedges_max),
# measured by test_vanilla_zoo_host.py and read back from the scratch struct on the GPU
STATS = {
    "asym": (9, 67, 401, 392),
    "deg": (19, 71, 449, 449),
    "deg17_2": (19, 71, 449, 449),
    "dense3": (11, 399, 2561, 2976),
    "dense4": (11, 399, 2561, 2976),
    "hub_tiled": (20, 1001, 1001, 339),
    "hub_untiled": (23, 1201, 1201, 339),  # (what the plan would be: it is refused)
    **{n: (6, 108, 369, 432) for n in WIDTH_BATCHES},
}
# ... and the kernels the pipeline then runs under its default knobs
# (``expected_path``; the PER_GRAPH_ONLY widths are within the chunk kernels'
# limits too, and only the per-graph test runs them on the GPU)
PATHS = {
    **{n: "chunk" for n in BATCHES},
    "hub_tiled": "tiled",
    "hub_untiled": "untiled",
    "w40_3": "tiled",
    "w64_8": "untiled",
    "w30_5": "untiled",
}


@functools.lru_cache(maxsize=None)
def datas(name):
    return tuple(BATCHES[name][2]())


def records(name):
    """The batch's per-graph records; Fe = 0 is a store without edge attributes."""
    recs = records_from_batch(graph_zoo.batch(datas(name)))
    if BATCHES[name][1] == 0:
        for r in recs:
            r.edge_attr = None
    return recs


@functools.lru_cache(maxsize=None)
def packed(name):
    return pack_graphs(records(name), require_clusters=False)


def is_symmetric(d):
    ei = d.edge_index.numpy()
    n = d.x.shape[0]
    return np.array_equal(np.sort(ei[0] * n + ei[1]), np.sort(ei[1] * n + ei[0]))


# --------------------------------------------------------------------------
# the tile plan and the dispatch rule, on the host
# --------------------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def plan(name, tile_rows=CHUNK, lds_check=True):
    """``vanilla_tile_plan`` of the whole batch from the packed arrays (a
    store on the CPU): (plan arrays as numpy, (n_tiles, hmax, emax, tmax), the
    tiles' dr_vanilla_tile fields), or None where the plan refuses."""
    p = packed(name)
    h = BatchHandle(GraphStore(p, "cpu"), np.arange(p.n_graphs))
    n = p.sizes()[0]
    row0 = np.concatenate([[0], np.cumsum(n)]).astype(np.int32)
    meta = []
    got = vanilla_tile_plan(h, n, row0, tile_rows, BATCHES[name][1], lds_check=lds_check, meta_out=meta)
    if got is None:
        return None
    tensors, stats = got
    return [t.numpy() for t in tensors], stats, meta


def _carve_total(kind, q):
    arr = (ctypes.c_int32 * len(q))(*q)
    buf = ctypes.create_string_buffer(8192)
    n = getattr(_lib.load(), f"dr_debug_carve_{kind}")(arr, buf, 8192)
    assert 0 < n < 8192  # noqa: PLR2004
    vals = dict(part.split("=") for part in buf.value.decode().split(";") if part)
    return 4 * int(vals["total"])


def carve_bytes(f, fe, hmax, emax, tmax):
    """LDS bytes of every kernel that stages a tile: the chunk-fused forward,
    the two chunk-fused backward edge kernels, the tiled edge kernels."""
    fes = max(fe, 1)
    return {
        "chunk_fwd": _carve_total("vanilla_chunk_fwd", (f, hmax, emax, fe)),
        "chunk_eb2": _carve_total("vanilla_chunk_bwd", (f, hmax, emax, tmax, fe, 1)),
        "chunk_eb1": _carve_total("vanilla_chunk_bwd", (f, hmax, emax, tmax, fe, 0)),
        "tile_fwd": _carve_total("vanilla_tile", (hmax, emax, tmax, fes, 0)),
        "tile_bwd": _carve_total("vanilla_tile", (hmax, emax, tmax, fes, 1)),
    }


def expected_path(f, fe, words, tile_rows, stats):
    """The kernels dr_vanilla_graph_pass runs, by its own rule restated:
    "chunk" (the vc_* kernels), "tiled" (vb_edge_*_tile) or "untiled".
    ``stats``: (n_tiles, hmax, emax, tmax) as measured without the plan's own
    LDS check."""
    if not words or not tile_rows or stats is None:
        return "untiled"
    c = carve_bytes(f, fe, *stats[1:])
    if max(c["tile_fwd"], c["tile_bwd"]) > LDS_MAX:  # vanilla_tile_plan returns None
        return "untiled"
    if tile_rows == CHUNK and fe <= 4 and f <= 32 and max(c["chunk_fwd"], c["chunk_eb2"], c["chunk_eb1"]) <= LDS_MAX:  # noqa: PLR2004
        return "chunk"
    return "tiled" if fe <= 4 else "untiled"  # noqa: PLR2004  (the generic edge kernels take no plan)


# --------------------------------------------------------------------------
# the oracle, and the tolerances against it
# --------------------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def oracle(name, loss="mse", dtype="f64", out_dim=None):
    """One forward + backward of ``oracle.gnn_ref.VanillaNetwork`` in float64
    or float32 from the same float32 initial weights and inputs: (state dict,
    outputs, loss, gradients by parameter name).  ``loss``: "mse" on the stored
    targets (1 output) or "ce" over 3 classes (targets i % 3).  ``out_dim``
    overrides the output count: "ce" then runs over that many classes (targets
    i % out_dim), and "mse" with more than one output is the project's
    multi-output rule restated from ``engine._layered_step`` and
    ``engine.loss_scale``: column 0 alone against the stored targets, summed
    and divided by B * out_dim."""
    f, fe, _ = BATCHES[name]
    if out_dim is None:
        out_dim = 1 if loss == "mse" else 3
    torch.manual_seed(SEEDS.get(name, 11))
    model = gnn_ref.VanillaNetwork(f, out_dim, fe)
    state = {k: v.detach().clone() for k, v in model.state_dict().items()}
    bat = graph_zoo.batch(datas(name))
    y = bat.y.clone()
    if dtype == "f64":
        model = model.double()
        bat.x, bat.edge_attr, y = bat.x.double(), bat.edge_attr.double(), y.double()
    out = model(bat)
    if loss == "mse" and out_dim == 1:
        lval = torch.nn.functional.mse_loss(out.reshape(-1), y)
    elif loss == "mse":
        lval = ((out[:, 0] - y) ** 2).sum() / (len(datas(name)) * out_dim)
    else:
        lval = torch.nn.functional.cross_entropy(out, torch.arange(len(datas(name))) % out_dim)
    lval.backward()
    grads = {n: p.grad.detach().numpy().copy() for n, p in model.named_parameters()}
    return state, out.detach().numpy(), float(lval.detach()), grads


OUT_TOL = dict(rtol=1e-4, atol=1e-4)
LOSS_RTOL = 1e-4
GRAD_RTOL, GRAD_NTOL, GRAD_CEILING = 1e-4, 1e-6, 1e-5


def grad_atol(ref64, ref32):
    """Absolute tolerance of a gradient against the float64 oracle, and the
    float32 oracle's own largest deviation from it.  The project's floor
    (``_util.assert_grad_close``: max(1e-6, 1e-6 max|ref|)); where the float32
    oracle itself deviates by more, up to 4 x that deviation (the kernel is a
    second float32 summation order of the same terms), never above the 1e-5
    max|ref| that test_gpu_mixed.py documents for the edge-MLP weight."""
    scale = float(np.abs(ref64).max()) if ref64.size else 0.0
    dev = float(np.abs(ref32.astype(np.float64) - ref64).max()) if ref64.size else 0.0
    base = max(1e-6, GRAD_NTOL * scale)
    return max(base, min(4.0 * dev, GRAD_CEILING * scale)), dev


def assert_grads_close(grads, name, loss, out_dim=None):
    """``grads`` (by parameter name) against the float64 oracle under
    ``grad_atol``; a failure lists the oracle's and the kernel's deviation of
    every parameter."""
    g64, g32 = oracle(name, loss, "f64", out_dim)[3], oracle(name, loss, "f32", out_dim)[3]
    lines, bad = [], []
    for n in PARAM_NAMES:
        got = np.asarray(grads[n], dtype=np.float64)
        atol, dev = grad_atol(g64[n], g32[n])
        err = np.abs(got - g64[n])
        lines.append(f"{n}: max|ref| {np.abs(g64[n]).max():.3g}  float32 oracle {dev:.3g}  kernel {err.max():.3g}  atol {atol:.3g}")
        if not (err <= atol + GRAD_RTOL * np.abs(g64[n])).all():
            bad.append(n)
    print("\n".join(lines))
    assert not bad, f"{name}/{loss}: {bad} outside tolerance\n" + "\n".join(lines)


# --------------------------------------------------------------------------
# one training step on the GPU against the oracle
# --------------------------------------------------------------------------

DEV = "cuda:0"


def handle(name, loss="mse", out_dim=None, **knobs):
    """A batch handle of the whole batch on a fresh GPU store ("ce": targets
    i % out_dim, 3 classes by default) with the knobs set."""
    p = packed(name)
    store = GraphStore(p, DEV)
    if loss == "ce":
        store.set_targets(np.arange(p.n_graphs) % (3 if out_dim is None else out_dim))
    h = BatchHandle(store, np.arange(p.n_graphs))
    for k, v in knobs.items():
        setattr(h, k, v)
    return h


def train_step(name, loss, pipeline=True, out_dim=None, got=None, **knobs):
    """One FusedTrainStep.step of the batch under the handle knobs: outputs,
    loss, gradients and the Adam update against the float64 oracle
    (``out_dim``: as ``oracle``).  ``got``: a dict that receives the step's
    "out", "loss" and "grads" (by parameter name) as numpy copies."""
    import pytest  # noqa: PLC0415

    from deeprank2_amd.engine import FusedTrainStep  # noqa: PLC0415
    from deeprank2_amd.neuralnets.gnn import vanilla_gnn as amd  # noqa: PLC0415

    f, fe, _ = BATCHES[name]
    state, out_o, loss_o, _ = oracle(name, loss, "f64", out_dim)
    h = handle(name, loss, out_dim, **knobs)
    if pipeline:
        h.vanilla_pipeline = True
    model = amd.VanillaNetwork(f, out_o.shape[1], fe)
    model.load_state_dict(state)
    step = FusedTrainStep(model.to(DEV).train(), loss=loss)
    before = [p.detach().clone() for p in step.params]
    loss_v, out = step.step(h)
    torch.cuda.synchronize()
    grads = {n: g.cpu().numpy() for n, g in zip(PARAM_NAMES, step.grads)}
    if got is not None:
        got.update(out=out.cpu().numpy().copy(), loss=float(loss_v), grads={n: g.copy() for n, g in grads.items()})
    np.testing.assert_allclose(out.cpu().numpy().astype(np.float64), out_o, **OUT_TOL)
    assert float(loss_v) == pytest.approx(loss_o, rel=LOSS_RTOL)
    assert_grads_close(grads, name, loss, out_dim)
    ref = [torch.nn.Parameter(b) for b in before]
    for r, g in zip(ref, step.grads):
        r.grad = g.detach().clone()
    torch.optim.Adam(ref, lr=1e-3, weight_decay=1e-5).step()
    for n, r, p in zip(PARAM_NAMES, ref, step.params):
        np.testing.assert_allclose(p.detach().cpu().numpy(), r.detach().cpu().numpy(), rtol=1e-5, atol=1e-7, err_msg=n)
    return h


# --------------------------------------------------------------------------
# the network restated in float64 on the packed and planned arrays
# --------------------------------------------------------------------------


def planned_columns(name, tile_rows=CHUNK):
    """Per graph: (CSR columns, transposed sources) read back through the tile
    plan, ``halo_ids[halo_off[t] + lcol]`` and ``... + ltcol``."""
    p = packed(name)
    (_, hoff, hids, loff, lcol, toff, ltcol), _, _ = plan(name, tile_rows, lds_check=False)
    lcol, ltcol = lcol.view(np.uint16), ltcol.view(np.uint16)
    out, t = [], 0
    for ng in p.sizes()[0]:
        cs, ts = [], []
        for _ in range(-(-int(ng) // tile_rows)):
            cs.append(hids[hoff[t] + lcol[loff[t] : loff[t + 1]].astype(np.int64)])
            ts.append(hids[hoff[t] + ltcol[toff[t] : toff[t + 1]].astype(np.int64)])
            t += 1
        out.append((np.concatenate(cs).astype(np.int64), np.concatenate(ts).astype(np.int64)))
    return out


def restated(name, params, columns=None, swap=False):
    """VanillaNetwork with MSE in float64 numpy, in the kernels' form: per
    layer A = X Wa^T, B = X Wb^T, S_i = sum over row i's CSR edges of
    relu(A_i + B_col + Wc ea + be); backward D_i over the CSR rows, D'_j over
    the transposed rows (sources ``t_col``, ReLU decisions through ``t_eid``).
    ``columns``: per graph (col, t_col), default the packed arrays'.  ``swap``:
    the transposed sum reads ``col`` where it needs ``t_col`` (the mix-up).
    Returns (outputs [B], loss, gradients by parameter name)."""
    p = packed(name)
    f = p.n_feat
    w = [np.asarray(q, dtype=np.float64) for q in params]
    n_all = p.sizes()[0]
    b = p.n_graphs
    grads = [np.zeros_like(q) for q in w]
    outs, saved = np.zeros(b), []
    for g in range(b):
        n0, ng, e0, e1 = int(p.node_off[g]), int(n_all[g]), int(p.edge_off[g]), int(p.edge_off[g + 1])
        rp, trp = (a[n0 + g : n0 + g + ng + 1].astype(np.int64) for a in (p.rowptr, p.t_rowptr))
        col, tcol = (p.col[e0:e1].astype(np.int64), p.t_col[e0:e1].astype(np.int64)) if columns is None else columns[g]
        src, tdst = np.repeat(np.arange(ng), np.diff(rp)), np.repeat(np.arange(ng), np.diff(trp))
        teid = p.t_eid[e0:e1].astype(np.int64)
        tsrc = col if swap else tcol
        ea = np.zeros((e1 - e0, 0)) if p.edge_attr is None else p.edge_attr[e0:e1].astype(np.float64)
        x = p.x[n0 : n0 + ng].astype(np.float64)
        layers = []
        for l in range(2):
            we, be, wn, bn = w[4 * l : 4 * l + 4]
            pre = x[src] @ we[:, :f].T + x[col] @ we[:, f : 2 * f].T + ea @ we[:, 2 * f :].T + be
            act = pre > 0
            s = np.zeros((ng, 32))
            np.add.at(s, src, pre * act)
            xo = np.maximum(np.concatenate([x, s], axis=1) @ wn.T + bn, 0.0)
            layers.append((x, s, act, xo))
            x = xo
        gm = x.mean(axis=0)
        hid = np.maximum(w[8] @ gm + w[9], 0.0)
        outs[g] = float((w[10] @ hid + w[11])[0])
        saved.append((src, tdst, tsrc, teid, ea, layers, gm, hid))
    loss = float(np.mean((outs - p.y.astype(np.float64)) ** 2))
    for g in range(b):
        src, tdst, tsrc, teid, ea, layers, gm, hid = saved[g]
        dout = np.array([2.0 * (outs[g] - float(p.y[g])) / b])
        grads[10] += np.outer(dout, hid)
        grads[11] += dout
        dh = (dout @ w[10]) * (hid > 0)
        grads[8] += np.outer(dh, gm)
        grads[9] += dh
        dx = np.tile((dh @ w[8]) / layers[1][3].shape[0], (layers[1][3].shape[0], 1))
        for l in (1, 0):
            we, wn = w[4 * l], w[4 * l + 2]
            x, s, act, xo = layers[l]
            du = dx * (xo > 0)
            dxs = du @ wn
            ds = dxs[:, f:]
            dpre = ds[src] * act
            d, dp = np.zeros_like(s), np.zeros_like(s)
            np.add.at(d, src, dpre)
            np.add.at(dp, tdst, ds[tsrc] * act[teid])
            grads[4 * l] += np.concatenate([d.T @ x, dp.T @ x, dpre.T @ ea], axis=1)
            grads[4 * l + 1] += d.sum(axis=0)
            grads[4 * l + 2] += du.T @ np.concatenate([x, s], axis=1)
            grads[4 * l + 3] += du.sum(axis=0)
            dx = dxs[:, :f] + d @ we[:, :f] + dp @ we[:, f : 2 * f]
    return outs, loss, dict(zip(PARAM_NAMES, grads))
