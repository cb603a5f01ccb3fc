"""Per-node attribution for GINet: the gradient of an output with respect to
the node features ``x`` — which residues, and which of their features, drove
a prediction.

``input_gradients`` returns what
``torch.autograd.grad((model(batch) * seed).sum(), batch.x)`` returns on the
reference model (``GINetConvLayer.forward`` ginet.py:40-60 under
``GINet.forward`` ginet.py:90-125), for any list of graphs of a resident
store, with one ``dr_ginet_input_grad_pass`` launch per batch: the training
pass's forward and backward, then ``dZ`` at the depth-0 pooling winners and
``dX = A^T dZ`` over the store's transposed CSR, all in the graph's workgroup.

GINetConvLayer's attention is a softmax over a size-1 dimension, identically
1 for finite inputs, so the gradient with respect to ``edge_attr`` is exactly
zero: nothing is computed or returned for it.

Batches the kernel does not take — a bf16 store, a graph flagged non-finite, a
graph beyond one workgroup's LDS, or ``fused=False`` — run
``layered.ginet_forward`` with ``x`` requiring grad and ``torch.autograd.grad``
(``result.path`` says which route the batches took).
"""

from __future__ import annotations

import copy
from dataclasses import dataclass

import numpy as np
import torch

from deeprank2_amd import _lib, layered
from deeprank2_amd.ensemble import _store_of
from deeprank2_amd.fused import LDS_MAX, BatchHandle, agg_x_for, make_pass
from deeprank2_amd.neuralnets.gnn import ginet

# Whether eligible batches run dr_ginet_input_grad_pass by default (the
# measurement behind the choice: DESIGN §5, profiles/attribution/)
FUSED_DEFAULT = True

SCORE_KINDS = ("l2", "l1", "grad_x_input")


@dataclass
class InputGradients:
    dx: torch.Tensor  # [rows, F] device view: d (out . seed) / d x, the requested graphs' nodes in order
    out: torch.Tensor  # [n, out_dim] eval-mode outputs of the requested graphs
    seed: torch.Tensor  # [n, out_dim] the upstream gradient each graph was seeded with
    node_off: np.ndarray  # host int64 [n + 1]: graph i's rows are node_off[i] .. node_off[i + 1] - 1
    indices: np.ndarray  # host int64 [n]: the graphs' positions in the store
    path: str  # "fused", "layers" or "mixed"

    def graph(self, i):
        """The rows of the i-th requested graph, ``[N_i, F]``."""
        return self.dx[int(self.node_off[i]) : int(self.node_off[i + 1])]


def batch_rows(n_nodes, indices, batch_size):
    """How the graphs ``indices`` (positions into a store whose graphs have
    ``n_nodes`` nodes) are cut and laid out: ``(batches, node_off)`` with
    ``batches`` the ``(start, stop)`` ranges of consecutive requested graphs,
    ``batch_size`` at a time (the last one may be short), and ``node_off``
    (int64 ``[n + 1]``) the first ``dx`` row of each requested graph — graph
    ``i`` of the request owns rows ``node_off[i] .. node_off[i + 1] - 1``
    whatever batch it runs in.  Pure host function."""
    if batch_size < 1:
        msg = f"batch_size must be positive (got {batch_size})"
        raise ValueError(msg)
    n_nodes = np.asarray(n_nodes, dtype=np.int64).reshape(-1)
    idx = np.asarray(indices, dtype=np.int64).reshape(-1)
    if idx.size and (idx.min() < 0 or idx.max() >= n_nodes.size):
        msg = f"a graph position lies outside the store's 0..{n_nodes.size - 1}"
        raise ValueError(msg)
    node_off = np.zeros(idx.size + 1, dtype=np.int64)
    np.cumsum(n_nodes[idx], out=node_off[1:])
    batches = [(s, min(s + batch_size, idx.size)) for s in range(0, idx.size, batch_size)]
    return batches, node_off


def _check_target(model, target, seed):
    """The refusals that need no device: the model class, and target / seed."""
    if type(model) is not ginet.GINet:
        msg = f"input_gradients supports GINet only (got {type(model).__name__})"
        raise NotImplementedError(msg)
    out_dim = int(model.output_shape)
    if target is not None and seed is not None:
        msg = "give target or seed, not both"
        raise ValueError(msg)
    if seed is not None:
        return
    if target is None:
        if out_dim != 1:
            msg = f"the model has {out_dim} outputs: name one with target (an index or 'pred') or pass seed"
            raise ValueError(msg)
    elif isinstance(target, str):
        if target != "pred":
            msg = f"target must be None, an output index or 'pred' (got {target!r})"
            raise ValueError(msg)
    elif isinstance(target, (bool, float)) or not isinstance(target, (int, np.integer)) or not 0 <= int(target) < out_dim:
        msg = f"target must lie in 0..{out_dim - 1} (got {target!r})"
        raise ValueError(msg)


def _one_hot_pred(out):
    """Each row's arg-max output as a one-hot seed, on the device."""
    return torch.zeros_like(out).scatter_(1, out.argmax(dim=1, keepdim=True), 1.0)


def _ig_lds(h: BatchHandle, out_dim, zs):
    alias, f = int(h.store.packed.transpose_aliased), h.store.n_feat
    return int(_lib.load().dr_ginet_input_grad_lds_bytes(*h.max_sizes[:2], f, *h.max_sizes[2:], alias, out_dim, zs))


def input_gradients(model, dataset, indices=None, batch_size=64, target=None, seed=None, fused=None, *, dx_out=None) -> InputGradients:
    """``d (out . seed) / d x`` for the graphs ``indices`` of ``dataset`` (a
    ``GraphDataset`` or a ``GraphStore``; positions into it, default all), in
    that order, in batches of ``batch_size``.

    ``model``: a ``GINet`` on the GPU, evaluated in eval mode (no dropout); its
    ``training`` flag, parameters and any optimizer state are not touched.
    ``target``: ``None`` (output 0 of a one-output model), an output index, or
    ``"pred"`` (each graph's arg-max output, from one forward first).  ``seed``:
    instead of ``target``, a ``[n, out_dim]`` tensor used as the upstream
    gradient.  ``fused``: ``False`` runs every batch on the layer path;
    default ``FUSED_DEFAULT``.  ``dx_out``: an fp32 device buffer of at least
    ``[rows, x_stride]`` to write into (default: a new one); rows past the
    request are left alone.

    One ``dx`` buffer ``[rows, x_stride]`` serves the whole call: every launch
    writes its graphs' rows in place (``dr_input_grad.row_off``); the scratch
    slab and head of the training pass are allocated once.  The gradient with
    respect to ``edge_attr`` is exactly zero (module docstring) and is not
    returned."""
    _check_target(model, target, seed)
    params = [p.detach().contiguous() for p in model.ordered_params()]
    dev = params[0].device
    if dev.type != "cuda":
        msg = "input_gradients runs on the MI355X only: move the model to a cuda device (no CPU fallback)"
        raise RuntimeError(msg)
    fused = FUSED_DEFAULT if fused is None else bool(fused)
    store = _store_of(dataset, dev)
    f, out_dim, xs = store.n_feat, int(model.output_shape), store.x_stride
    if f != model.input_shape:
        msg = f"the store has {f} node features, model expects {model.input_shape}"
        raise ValueError(msg)
    idx = np.arange(store.n_graphs, dtype=np.int64) if indices is None else np.asarray(indices, dtype=np.int64).reshape(-1)
    batches, node_off = batch_rows(store._sizes[0], idx, batch_size)  # noqa: SLF001
    n, rows = int(idx.size), int(node_off[-1])

    if seed is not None:
        seed_t = torch.as_tensor(seed, dtype=torch.float32, device=dev).contiguous()
        if tuple(seed_t.shape) != (n, out_dim):
            msg = f"seed must be [{n}, {out_dim}] (got {list(seed_t.shape)})"
            raise ValueError(msg)
        seed_t = seed_t.clone()
    else:
        seed_t = torch.zeros(n, out_dim, dtype=torch.float32, device=dev)
        if target != "pred":
            seed_t[:, 0 if target is None else int(target)] = 1.0

    if dx_out is None:
        dx_buf = torch.empty((max(rows, 1), xs), dtype=torch.float32, device=dev)
    else:
        dx_buf = dx_out
        if dx_buf.dtype != torch.float32 or dx_buf.device != dev or dx_buf.dim() != 2 or dx_buf.shape[1] != xs or dx_buf.shape[0] < rows or not dx_buf.is_contiguous():  # noqa: PLR2004
            msg = f"dx_out must be a contiguous fp32 [>= {rows}, {xs}] tensor on {dev}"
            raise ValueError(msg)
    out = torch.empty(n, out_dim, dtype=torch.float32, device=dev)
    row_off = torch.from_numpy(node_off[:-1].copy()).to(dev) if n else None
    w = ginet.weights_c(params)
    bmax = max((e - s for s, e in batches), default=0)
    slab = head = None  # the training pass's partials: scratch here, made on the first fused batch
    lib = _lib.load()
    taken = set()
    for s, e in batches:
        h = BatchHandle(store, idx[s:e].astype(np.int32))
        z = agg_x_for(ginet.SPEC, h) if fused and store.dtype != "bf16" else None
        zs = store.agg_x_stride if z is not None else 0
        if fused and store.dtype != "bf16" and not h.nonfinite and _ig_lds(h, out_dim, zs) <= LDS_MAX:
            if slab is None:
                slab = torch.empty(bmax * ginet.slab_stride(f), dtype=torch.float32, device=dev)
                head = torch.zeros(bmax * ginet.head_stride(out_dim), dtype=torch.float32, device=dev)
            if target == "pred":  # one forward through the eval path, then the one-hot on the device
                ginet.graph_pass(h, params, out_dim, _lib.DR_PASS_FORWARD, out=out[s:e])
                seed_t[s:e] = _one_hot_pred(out[s:e])
            p = make_pass(out_dim, _lib.DR_PASS_FORWARD | _lib.DR_PASS_BACKWARD, dout=seed_t[s:e], out=out[s:e], slab=slab, head=head)
            ig = _lib.InputGradC()
            ig.dx, ig.row_off, ig.dx_stride = dx_buf.data_ptr(), row_off.data_ptr() + 8 * s, xs
            rc = lib.dr_ginet_input_grad_pass(store.cstruct(), h.descs.data_ptr(), h.B, w, p, ig, _lib.ptr(z), zs, _ig_lds(h, out_dim, zs), _lib.stream_ptr(dev))
            _lib.check(rc, "dr_ginet_input_grad_pass")
            taken.add("fused")
        else:
            t = copy.copy(layered.batch_tensors(h))
            t.x = t.x.detach().clone().requires_grad_(True)
            with torch.enable_grad():
                o = layered.ginet_forward(model, t, training=False)
                if target == "pred":
                    seed_t[s:e] = _one_hot_pred(o.detach())
                (g,) = torch.autograd.grad((o * seed_t[s:e]).sum(), t.x)
            out[s:e] = o.detach()
            r0, r1 = int(node_off[s]), int(node_off[e])
            dx_buf[r0:r1, :f] = g
            dx_buf[r0:r1, f:] = 0.0
            taken.add("layers")
    path = "mixed" if len(taken) > 1 else (taken.pop() if taken else ("fused" if fused else "layers"))
    return InputGradients(dx_buf[:rows, :f], out, seed_t, node_off, idx, path)


def _rows_of(result: InputGradients, store):
    """The store rows of the result's nodes, in the result's order (device int64)."""
    off = np.asarray(store.packed.node_off, dtype=np.int64)
    parts = [np.arange(off[g], off[g + 1], dtype=np.int64) for g in result.indices]
    rows = np.concatenate(parts) if parts else np.zeros(0, np.int64)
    return torch.from_numpy(rows).to(result.dx.device)


def node_scores(result: InputGradients, store_or_dataset, kind="l2"):
    """One score per node of the result (device ``[rows]``): ``"l2"``
    (sqrt of sum_f dx^2), ``"l1"`` (sum_f |dx|) or ``"grad_x_input"`` (sum_f x * dx,
    signed), by plain torch on the device."""
    if kind not in SCORE_KINDS:
        msg = f"kind must be one of {SCORE_KINDS} (got {kind!r})"
        raise ValueError(msg)
    dx = result.dx
    if kind == "l2":
        return dx.square().sum(dim=1).sqrt()
    if kind == "l1":
        return dx.abs().sum(dim=1)
    store = _store_of(store_or_dataset, dx.device)
    x = store.x[_rows_of(result, store), : dx.shape[1]]
    return (x * dx).sum(dim=1)


def top_nodes(result: InputGradients, scores, i, k):
    """Host indices (local node ids, int64) of the ``k`` highest-scoring nodes
    of the i-th requested graph, highest first; equal scores in node order."""
    s = scores[int(result.node_off[i]) : int(result.node_off[i + 1])].detach().cpu().numpy()
    return np.argsort(-s, kind="stable")[: max(0, int(k))].astype(np.int64)
