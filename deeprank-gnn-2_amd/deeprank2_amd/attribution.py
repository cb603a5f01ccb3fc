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

``integrated_gradients`` integrates that gradient along the straight path from
a baseline to ``x`` (Sundararajan et al. 2017): on the reference model, one
``torch.autograd.grad`` per quadrature node, weighted and summed, times
``x - baseline`` (the reference has no attribution call of its own).  Conv1
aggregates first and ``Z = A x`` is linear in ``x``, so every node of the path
is the Z-input pass on a rescaled Z block, and one
``dr_ginet_integrated_grad_pass`` runs all of them for a batch; the layer route
runs the steps one by one for the batches that pass does not take.
"""

from __future__ import annotations

import copy
import functools
from dataclasses import dataclass

import numpy as np
import torch

from deeprank2_amd import _lib, layered
from deeprank2_amd.ensemble import _store_of
from deeprank2_amd.fused import LDS_MAX, BatchHandle, agg_x_for, make_pass, z_lds_for
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


# ---------------------------------------------------------------------------
# Integrated gradients
# ---------------------------------------------------------------------------

# Workgroups per graph of dr_ginet_integrated_grad_pass when ``groups`` is not
# given: the fastest of {1, 2, 4, 8, 32} at 32 steps on a batch of 64 (DESIGN §5,
# profiles/integrated_gradients/bench_ig.txt); capped by the step count, never
# by the batch, so a graph gets the same bits alone and inside a batch.
IG_GROUPS_DEFAULT = 4

QUADRATURES = ("gausslegendre", "midpoint")


def quadrature(method, steps):
    """The nodes ``alpha`` (ascending, strictly inside (0, 1)) and weights
    (sum 1) of an ``steps``-point rule on [0, 1], float64: ``"gausslegendre"``
    (``numpy.polynomial.legendre.leggauss`` mapped from [-1, 1]) or
    ``"midpoint"`` (``(s + 1/2) / steps``, ``1 / steps``).  Pure host function."""
    if isinstance(steps, bool) or not isinstance(steps, (int, np.integer)) or steps < 1:
        msg = f"steps must be a positive integer (got {steps!r})"
        raise ValueError(msg)
    steps = int(steps)
    if method == "gausslegendre":
        t, w = np.polynomial.legendre.leggauss(steps)
        return 0.5 * (t + 1.0), 0.5 * w
    if method == "midpoint":
        return (np.arange(steps, dtype=np.float64) + 0.5) / steps, np.full(steps, 1.0 / steps)
    msg = f"method must be one of {QUADRATURES} (got {method!r})"
    raise ValueError(msg)


@functools.lru_cache(maxsize=32)
def _quadrature_cached(method, steps):
    """``quadrature`` once per rule (``leggauss`` is an eigenvalue problem on the host)."""
    return quadrature(method, steps)


@dataclass
class IntegratedGradients:
    attr: torch.Tensor  # [rows, F] device view: (x - baseline) * sum_s w_s g_s, the requested graphs' nodes in order
    out: torch.Tensor  # [n, out_dim] eval-mode outputs at x
    out_baseline: torch.Tensor  # [n, out_dim] eval-mode outputs at the baseline
    seed: torch.Tensor  # [n, out_dim] the upstream gradient each graph was seeded with
    attr_sum: torch.Tensor  # [n] fp64: each graph's sum of attr
    delta: torch.Tensor  # [n] fp64: attr_sum - (out - out_baseline) . seed, the completeness gap (quadrature error)
    node_off: np.ndarray  # host int64 [n + 1]: graph i's rows are node_off[i] .. node_off[i + 1] - 1
    indices: np.ndarray  # host int64 [n]: the graphs' positions in the store
    path: str  # "fused", "layers" or "mixed"
    alpha: np.ndarray  # host fp32 [steps]: the quadrature nodes the device used
    weight: np.ndarray  # host fp32 [steps]: the quadrature weights the device used

    @property
    def dx(self):
        """``attr`` under the name ``node_scores`` / ``top_nodes`` read."""
        return self.attr

    def node_attr(self):
        """The signed attribution of each node, ``[rows]``: its features' sum."""
        return self.attr.sum(dim=1)

    def graph(self, i):
        """The rows of the i-th requested graph, ``[N_i, F]``."""
        return self.attr[int(self.node_off[i]) : int(self.node_off[i + 1])]


def _store_rows(store, gids):
    """Host int64: the store rows of the nodes of graphs ``gids``, in that order."""
    off = np.asarray(store.packed.node_off, dtype=np.int64)
    parts = [np.arange(off[g], off[g + 1], dtype=np.int64) for g in gids]
    return np.concatenate(parts) if parts else np.zeros(0, np.int64)


def _intgrad_lds(h: BatchHandle, out_dim, zs):
    alias, f = int(h.store.packed.transpose_aliased), h.store.n_feat
    return int(_lib.load().dr_ginet_integrated_grad_lds_bytes(*h.max_sizes[:2], f, *h.max_sizes[2:], alias, out_dim, zs))


def _forward_z(h: BatchHandle, w, out_dim, z, zs, out):
    """The eval forward of the Z-input entry on the array ``z`` (Z = A x, or A b for a baseline)."""
    p = make_pass(out_dim, _lib.DR_PASS_FORWARD, out=out)
    rc = _lib.load().dr_ginet_graph_pass_z(h.store.cstruct(), h.descs.data_ptr(), h.B, w, p, z_lds_for(h, out_dim), z.data_ptr(), zs, _lib.stream_ptr(h.store.device))
    _lib.check(rc, "dr_ginet_graph_pass_z")


def _check_ig_args(model, steps, method, groups, baseline, quad):
    """The refusals of ``integrated_gradients`` beyond ``_check_target`` that
    need no device; returns (alpha, weight) as fp32 arrays and the group count."""
    if quad is not None:
        alpha, weight = (np.asarray(v, dtype=np.float64).reshape(-1) for v in quad)
        if alpha.size < 1 or alpha.size != weight.size:
            msg = "the nodes and the weights must be two equally long, non-empty vectors"
            raise ValueError(msg)
    else:
        plain = isinstance(method, str) and isinstance(steps, (int, np.integer)) and not isinstance(steps, bool)
        alpha, weight = _quadrature_cached(method, int(steps)) if plain else quadrature(method, steps)  # (the refusals come from quadrature itself)
    n_steps = int(alpha.size)
    if groups is None:
        groups = min(IG_GROUPS_DEFAULT, n_steps)
    elif isinstance(groups, bool) or not isinstance(groups, (int, np.integer)) or not 1 <= groups <= n_steps:
        msg = f"groups must lie in 1..{n_steps}, the step count (got {groups!r})"
        raise ValueError(msg)
    if baseline is not None:
        shape = tuple(np.shape(baseline))
        if len(shape) not in (1, 2) or shape[-1] != model.input_shape:
            msg = f"baseline must be [{model.input_shape}] or [rows, {model.input_shape}] (got {list(shape)})"
            raise ValueError(msg)
    return alpha.astype(np.float32), weight.astype(np.float32), int(groups)


def integrated_gradients(model, dataset, indices=None, batch_size=64, target=None, seed=None, baseline=None, steps=32, method="gausslegendre", groups=None, fused=None, *, attr_out=None, _quadrature=None) -> IntegratedGradients:
    """Integrated gradients (Sundararajan et al. 2017) of ``out . seed`` with
    respect to the node features, for the graphs ``indices`` of ``dataset``:

        attr[i, f] = (x[i, f] - b[i, f]) * sum_s w_s g_s[i, f],
        g_s = d (out(x_s) . seed) / dx  at  x_s = b + alpha_s (x - b),

    with ``(alpha, w) = quadrature(method, steps)`` rounded to fp32.  The
    attributions of a graph sum to ``(out - out_baseline) . seed`` up to the
    quadrature's error, which ``delta`` reports per graph.

    ``model``, ``dataset``, ``indices``, ``batch_size``, ``target``, ``seed``,
    ``fused``: as :func:`input_gradients` (``"pred"`` is decided once, from the
    forward at ``x``).  ``baseline``: ``None`` (zeros: the dataset mean of
    standardised features), an ``[F]`` vector given to every node, or a
    ``[rows, F]`` tensor in the request's node order (no graph may then be
    requested twice).  ``groups``: workgroups per graph of the fused pass, each
    taking a contiguous range of the steps (default ``IG_GROUPS_DEFAULT``, at
    most ``steps``).  ``attr_out``: as ``input_gradients``' ``dx_out``.

    Eligible batches — an fp32 store with its Z = A x array, no non-finite
    graph, ``dr_ginet_integrated_grad_lds_bytes`` within one workgroup's LDS —
    take three launches: the Z-input forward at ``x``, the same at the baseline
    (a zero baseline: the closed form ``fc2(relu(fc1.bias))``) and
    ``dr_ginet_integrated_grad_pass``.  The others run ``steps`` times
    ``layered.ginet_forward`` + ``torch.autograd.grad`` with the same nodes and
    weights.  The ``edge_attr`` attribution is exactly zero (module docstring)
    and is not returned."""
    _check_target(model, target, seed)
    alpha, weight, n_groups = _check_ig_args(model, steps, method, groups, baseline, _quadrature)
    n_steps = int(alpha.size)
    params = [p.detach().contiguous() for p in model.ordered_params()]
    dev = params[0].device
    if dev.type != "cuda":
        msg = "integrated_gradients runs on the MI355X only: move the model to a cuda device (no CPU fallback)"
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

    if attr_out is None:
        attr_buf = torch.empty((max(rows, 1), xs), dtype=torch.float32, device=dev)
    else:
        attr_buf = attr_out
        if attr_buf.dtype != torch.float32 or attr_buf.device != dev or attr_buf.dim() != 2 or attr_buf.shape[1] != xs or attr_buf.shape[0] < rows or not attr_buf.is_contiguous():  # noqa: PLR2004
            msg = f"attr_out must be a contiguous fp32 [>= {rows}, {xs}] tensor on {dev}"
            raise ValueError(msg)

    lib = _lib.load()
    stream = _lib.stream_ptr(dev)
    z_all = store.agg_x() if fused and store.dtype != "bf16" else None
    zs = store.agg_x_stride
    # the baseline in x's layout and its neighbour sums in Z's, once per call
    xb = zb = None
    if baseline is not None:
        b_t = torch.as_tensor(baseline, dtype=torch.float32, device=dev)
        xb = torch.zeros((max(1, int(store.x.shape[0])), xs), dtype=torch.float32, device=dev)
        if b_t.dim() == 1:
            xb[:, :f] = b_t
        else:
            if b_t.shape[0] != rows:
                msg = f"baseline must be [{f}] or [{rows}, {f}] (got {list(b_t.shape)})"
                raise ValueError(msg)
            if np.unique(idx).size != idx.size:
                msg = "a per-node baseline needs every requested graph named once"
                raise ValueError(msg)
            xb[torch.from_numpy(_store_rows(store, idx)).to(dev), :f] = b_t
        if z_all is not None:
            zb = torch.empty_like(z_all)
            st = _lib.GraphStoreC.from_buffer_copy(store.cstruct())
            st.x = xb.data_ptr()
            _lib.check(lib.dr_aggregate_x(st, zb.data_ptr(), zs, 0, store.n_graphs, stream), "dr_aggregate_x")

    out = torch.empty(n, out_dim, dtype=torch.float32, device=dev)
    out_b = torch.empty(n, out_dim, dtype=torch.float32, device=dev)
    attr_sum = torch.zeros(n, dtype=torch.float64, device=dev)
    w = ginet.weights_c(params)
    bmax = max((e - s for s, e in batches), default=0)
    rmax = max((int(node_off[e] - node_off[s]) for s, e in batches), default=0)
    offs = None  # [2, n]: each graph's first row of attr, and its first row inside its batch (the partial rows)
    if n:
        first = np.repeat(node_off[[s for s, _ in batches]], [e - s for s, e in batches])
        offs = torch.from_numpy(np.stack([node_off[:-1], node_off[:-1] - first])).to(dev)
    quad_t = torch.from_numpy(np.stack([alpha, weight])).to(dev)  # [2, S]
    out_b0 = None  # a zero baseline's outputs: Z = 0 pools to zero features, so the head on a zero vector
    scratch = None  # per-group slab / head / out of the training pass and the partial rows, made on the first fused batch
    taken = set()
    for s, e in batches:
        h = BatchHandle(store, idx[s:e].astype(np.int32))
        lds = _intgrad_lds(h, out_dim, zs) if z_all is not None else -1
        if z_all is not None and not h.nonfinite and 0 <= lds <= LDS_MAX:
            if scratch is None:
                scratch = (
                    torch.empty(n_groups * bmax * ginet.slab_stride(f), dtype=torch.float32, device=dev),
                    torch.zeros(n_groups * bmax * ginet.head_stride(out_dim), dtype=torch.float32, device=dev),
                    torch.empty(n_groups * bmax * out_dim, dtype=torch.float32, device=dev),
                    torch.empty((n_groups, max(rmax, 1), xs), dtype=torch.float32, device=dev),
                )
            _forward_z(h, w, out_dim, z_all, zs, out[s:e])
            if zb is not None:
                _forward_z(h, w, out_dim, zb, zs, out_b[s:e])
            else:
                if out_b0 is None:
                    out_b0 = torch.relu(params[13]) @ params[14].t() + params[15]
                out_b[s:e] = out_b0
            if target == "pred":
                seed_t[s:e] = _one_hot_pred(out[s:e])
            p = make_pass(out_dim, _lib.DR_PASS_FORWARD | _lib.DR_PASS_BACKWARD, dout=seed_t[s:e])
            ig = _lib.IntegratedGradC()
            ig.attr, ig.row_off, ig.dx_stride = attr_buf.data_ptr(), offs.data_ptr() + 8 * s, xs
            ig.n_steps, ig.n_groups = n_steps, n_groups
            ig.alpha, ig.weight = quad_t.data_ptr(), quad_t.data_ptr() + 4 * n_steps
            ig.zb, ig.xb = _lib.ptr(zb), _lib.ptr(xb) if zb is not None else None
            ig.part, ig.part_off, ig.part_rows = scratch[3].data_ptr(), offs.data_ptr() + 8 * (n + s), scratch[3].shape[1]
            ig.attr_sum = attr_sum.data_ptr() + 8 * s
            ig.slab, ig.head, ig.out = scratch[0].data_ptr(), scratch[1].data_ptr(), scratch[2].data_ptr()
            rc = lib.dr_ginet_integrated_grad_pass(store.cstruct(), h.descs.data_ptr(), h.B, w, p, ig, z_all.data_ptr(), zs, lds, stream)
            _lib.check(rc, "dr_ginet_integrated_grad_pass")
            taken.add("fused")
        else:
            t = copy.copy(layered.batch_tensors(h))
            x0 = t.x.detach()
            if xb is None:
                b0 = torch.zeros_like(x0)
            else:
                b0 = xb[torch.from_numpy(_store_rows(store, idx[s:e])).to(dev), :f]
            with torch.no_grad():
                o = layered.ginet_forward(model, t, training=False)
                t.x = b0
                out_b[s:e] = layered.ginet_forward(model, t, training=False)
            out[s:e] = o
            if target == "pred":
                seed_t[s:e] = _one_hot_pred(o)
            acc = torch.zeros_like(x0)
            for k in range(n_steps):
                t.x = (b0 + float(alpha[k]) * (x0 - b0)).requires_grad_(True)
                with torch.enable_grad():
                    ok = layered.ginet_forward(model, t, training=False)
                    (g,) = torch.autograd.grad((ok * seed_t[s:e]).sum(), t.x)
                acc += float(weight[k]) * g
            a = (x0 - b0) * acc
            r0, r1 = int(node_off[s]), int(node_off[e])
            attr_buf[r0:r1, :f] = a
            attr_buf[r0:r1, f:] = 0.0
            attr_sum[s:e] = torch.zeros(e - s, dtype=torch.float64, device=dev).index_add_(0, t.batch.long(), a.double().sum(dim=1))
            taken.add("layers")
    path = "mixed" if len(taken) > 1 else (taken.pop() if taken else ("fused" if fused else "layers"))
    delta = attr_sum - ((out.double() - out_b.double()) * seed_t.double()).sum(dim=1)
    return IntegratedGradients(attr_buf[:rows, :f], out, out_b, seed_t, attr_sum, delta, node_off, idx, path, alpha, weight)


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
