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

Graphs beyond one workgroup's LDS (atom-level graphs) have a fused route of
their own, ``dr_ginet_large_input_grad_pass``: the large-graph path's tile
kernel and per-graph tail, ``dZ`` formed by the tail in a global workspace, and
a tile kernel for ``dX = A^T dZ``; the same bits as the single-workgroup pass on
graphs both take.  It is opt-in (``input_gradients(..., tiles=True)``,
``TILES_DEFAULT``).

``integrated_gradients`` integrates that gradient along the straight path from
a baseline to ``x`` (Sundararajan et al. 2017): on the reference model, one
``torch.autograd.grad`` per quadrature node, weighted and summed, times
``x - baseline`` (the reference has no attribution call of its own).  Conv1
aggregates first and ``Z = A x`` is linear in ``x``, so every node of the path
is the Z-input pass on a rescaled Z block, and one
``dr_ginet_integrated_grad_pass`` runs all of them for a batch; the layer route
runs the steps one by one for the batches that pass does not take.  Graphs
beyond one workgroup's LDS have the tile route here too
(``integrated_gradients(..., tiles=True)``,
``dr_ginet_large_integrated_grad_pass``): every step is the large-graph path's
tile kernel on the rescaled Z and its tail, the steps' ``dZ`` are summed in a
global workspace per group of steps and gathered once; the same bits as the
single-workgroup pass on graphs both take.
"""

from __future__ import annotations

import copy
import functools
from dataclasses import dataclass
from types import SimpleNamespace

import numpy as np
import torch

from deeprank2_amd import _lib, layered
from deeprank2_amd.fused import LDS_MAX, BatchHandle, agg_x_for, make_pass, z_lds_for
from deeprank2_amd.neuralnets.gnn import ginet
from deeprank2_amd.store import store_of

# Whether eligible batches run dr_ginet_input_grad_pass by default (the
# measurement behind the choice: DESIGN §5, profiles/attribution/)
FUSED_DEFAULT = True

# Whether batches beyond one workgroup's LDS run dr_ginet_large_input_grad_pass
# by default (opt-in until the default is decided on DESIGN §5 "Input gradients
# on tiles", profiles/attribution_large/)
TILES_DEFAULT = False
K0_TILES_MAX = 64  # most depth-0 clusters of a graph on the large-graph path (LargePlan)

SCORE_KINDS = ("l2", "l1", "grad_x_input")


class _NodeRows:
    """What the two results share: where a requested graph's rows lie in ``dx``."""

    def rows(self, i):
        """The i-th requested graph's rows of ``dx`` (and of any per-node score), as a slice."""
        return slice(int(self.node_off[i]), int(self.node_off[i + 1]))

    def graph(self, i):
        """The rows of the i-th requested graph, ``[N_i, F]``."""
        return self.dx[self.rows(i)]


@dataclass
class InputGradients(_NodeRows):
    dx: torch.Tensor  # [rows, F] device view: d (out . seed) / d x, the requested graphs' nodes in order
    out: torch.Tensor  # [n, out_dim] eval-mode outputs of the requested graphs
    seed: torch.Tensor  # [n, out_dim] the upstream gradient each graph was seeded with
    node_off: np.ndarray  # host int64 [n + 1]: graph i's rows are node_off[i] .. node_off[i + 1] - 1
    indices: np.ndarray  # host int64 [n]: the graphs' positions in the store
    path: str  # "fused", "tiles", "layers" or "mixed" (more than one route)


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


def _check_target(name, model, target, seed):
    """The refusals of the call ``name`` that need no device: the model class, and target / seed."""
    if type(model) is not ginet.GINet:
        msg = f"{name} supports GINet only (got {type(model).__name__})"
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


def _check_tiles(tiles):
    """``input_gradients``' ``tiles`` as False, True or "force" (needs no device)."""
    if tiles is None:
        tiles = TILES_DEFAULT
    if tiles is True or tiles is False or (isinstance(tiles, str) and tiles == "force"):
        return tiles
    msg = f"tiles must be None, False, True or 'force' (got {tiles!r})"
    raise ValueError(msg)


def _one_hot_pred(out):
    """Each row's arg-max output as a one-hot seed, on the device."""
    return torch.zeros_like(out).scatter_(1, out.argmax(dim=1, keepdim=True), 1.0)


def _lds(entry, h: BatchHandle, out_dim, zs):
    """Dynamic LDS bytes of the kernel whose query is ``entry`` for the batch's largest graph (-1: no such form), asked once per handle."""
    alias, f = int(h.store.packed.transpose_aliased), h.store.n_feat
    return h.lds((entry, out_dim, zs), lambda n, e, k0, p1, k1: getattr(_lib.load(), entry)(n, e, f, k0, p1, k1, alias, out_dim, zs))


def _store_rows(store, gids, dev):
    """The store rows of the nodes of graphs ``gids``, in that order (device int64)."""
    off = np.asarray(store.packed.node_off, dtype=np.int64)
    parts = [np.arange(off[g], off[g + 1], dtype=np.int64) for g in gids]
    return torch.from_numpy(np.concatenate(parts) if parts else np.zeros(0, np.int64)).to(dev)


class _Request:
    """One call of the public function ``name``, checked and laid out: the
    store and the weights, the requested graphs cut into batches
    (:func:`batch_rows`), the seed, and the buffers every batch writes its part
    of: ``buf`` (the caller's argument ``buf_name``, or a new one) and ``out``."""

    def __init__(self, name, model, dataset, indices, batch_size, target, seed, fused, buf, buf_name):
        self.model, self.target = model, target
        self.params = [p.detach().contiguous() for p in model.ordered_params()]
        self.dev = dev = self.params[0].device
        if dev.type != "cuda":
            msg = f"{name} runs on the MI355X only: move the model to a cuda device (no CPU fallback)"
            raise RuntimeError(msg)
        self.fused = FUSED_DEFAULT if fused is None else bool(fused)
        self.store = store = store_of(dataset, dev)
        self.f, self.out_dim, self.xs = store.n_feat, int(model.output_shape), store.x_stride
        if self.f != model.input_shape:
            msg = f"the store has {self.f} node features, model expects {model.input_shape}"
            raise ValueError(msg)
        self.kernel_ok = self.fused and store.dtype != "bf16"  # a bf16 store takes the layer route
        self.idx = np.arange(store.n_graphs, dtype=np.int64) if indices is None else np.asarray(indices, dtype=np.int64).reshape(-1)
        self.batches, self.node_off = batch_rows(store._sizes[0], self.idx, batch_size)  # noqa: SLF001
        self.n, self.rows = n, rows = int(self.idx.size), int(self.node_off[-1])
        if seed is not None:
            seed_t = torch.as_tensor(seed, dtype=torch.float32, device=dev).contiguous()
            if tuple(seed_t.shape) != (n, self.out_dim):
                msg = f"seed must be [{n}, {self.out_dim}] (got {list(seed_t.shape)})"
                raise ValueError(msg)
            self.seed_t = seed_t.clone()
        else:
            self.seed_t = torch.zeros(n, self.out_dim, dtype=torch.float32, device=dev)
            if target != "pred":
                self.seed_t[:, 0 if target is None else int(target)] = 1.0
        if buf is None:
            buf = torch.empty((max(rows, 1), self.xs), dtype=torch.float32, device=dev)
        elif buf.dtype != torch.float32 or buf.device != dev or buf.dim() != 2 or buf.shape[1] != self.xs or buf.shape[0] < rows or not buf.is_contiguous():  # noqa: PLR2004
            msg = f"{buf_name} must be a contiguous fp32 [>= {rows}, {self.xs}] tensor on {dev}"
            raise ValueError(msg)
        self.buf, self.view = buf, buf[:rows, : self.f]  # [>= rows, x_stride], and the result's [rows, F] view of it
        self.out = torch.empty(n, self.out_dim, dtype=torch.float32, device=dev)
        self.w = ginet.weights_c(self.params)
        self.bmax = max((e - s for s, e in self.batches), default=0)
        self.taken = set()  # the routes the batches took

    def handle(self, s, e):
        return BatchHandle(self.store, self.idx[s:e].astype(np.int32))

    def row_range(self, s, e):
        """The rows of ``buf`` that the batch of requested graphs ``s .. e - 1`` owns."""
        return int(self.node_off[s]), int(self.node_off[e])

    def write_rows(self, s, e, g):
        """A layer-route result ``g`` ``[rows of the batch, F]`` into the batch's rows, the pad columns zeroed."""
        r0, r1 = self.row_range(s, e)
        self.buf[r0:r1, : self.f] = g
        self.buf[r0:r1, self.f :] = 0.0

    def path(self):
        return "mixed" if len(self.taken) > 1 else (next(iter(self.taken)) if self.taken else ("fused" if self.fused else "layers"))


def _layer_grad(model, t, x, seed, pred=False):
    """The layer route's kernel: ``layered.ginet_forward`` on the batch tensors
    ``t`` at ``t.x = x``, and ``torch.autograd.grad``: the detached outputs and
    ``d (out . seed) / d x``.  ``pred`` first makes ``seed`` (the caller's view) that forward's one-hot arg-max."""
    t.x = x.requires_grad_(True)
    with torch.enable_grad():
        o = layered.ginet_forward(model, t, training=False)
        if pred:
            seed[:] = _one_hot_pred(o.detach())
        (g,) = torch.autograd.grad((o * seed).sum(), t.x)
    return o.detach(), g


def _input_grad_args(rq: _Request, c, h: BatchHandle, s, e):
    """What the two fused routes hand their entry alike: the pass (seeded; for
    ``"pred"`` after one forward through the eval path and the one-hot on the
    device) and the ``dr_input_grad`` of the batch's rows."""
    out_dim, dev = rq.out_dim, rq.dev
    if c.slab is None:
        c.slab = torch.empty(rq.bmax * ginet.slab_stride(rq.f), dtype=torch.float32, device=dev)
        c.head = torch.zeros(rq.bmax * ginet.head_stride(out_dim), dtype=torch.float32, device=dev)
    if rq.target == "pred":
        ginet.graph_pass(h, rq.params, out_dim, _lib.DR_PASS_FORWARD, out=rq.out[s:e])
        rq.seed_t[s:e] = _one_hot_pred(rq.out[s:e])
    p = make_pass(out_dim, _lib.DR_PASS_FORWARD | _lib.DR_PASS_BACKWARD, dout=rq.seed_t[s:e], out=rq.out[s:e], slab=c.slab, head=c.head)
    ig = _lib.InputGradC()
    ig.dx, ig.row_off, ig.dx_stride = rq.buf.data_ptr(), c.row_off.data_ptr() + 8 * s, rq.xs
    return p, ig


def _input_grad_fused(rq: _Request, c, h: BatchHandle, s, e, z, zs):
    """One ``dr_ginet_input_grad_pass`` launch: the batch's rows of ``dx`` in place."""
    out_dim, dev = rq.out_dim, rq.dev
    p, ig = _input_grad_args(rq, c, h, s, e)
    lds = _lds("dr_ginet_input_grad_lds_bytes", h, out_dim, zs)
    rc = _lib.load().dr_ginet_input_grad_pass(rq.store.cstruct(), h.descs.data_ptr(), h.B, rq.w, p, ig, _lib.ptr(z), zs, lds, _lib.stream_ptr(dev))
    _lib.check(rc, "dr_ginet_input_grad_pass")


def _tile_plan(rq: _Request, h: BatchHandle):
    """The batch's ``dr_large_plan`` if it passes the tile checks (an fp32
    store on the fused route, no non-finite graph, every graph within
    ``K0_TILES_MAX`` clusters, the plan's LDS within one workgroup's), else None."""
    if not rq.kernel_ok or h.nonfinite or h.max_sizes[2] > K0_TILES_MAX:
        return None
    try:
        return h.large_plan(rq.out_dim)
    except RuntimeError:  # LargePlan's refusal: a tile or the tail beyond 160 KiB of LDS
        return None


def _route(tiles, plan, fits):
    """The route of one batch, ``"tiles"``, ``"fused"`` or ``"layers"``, from
    ``tiles`` (checked), the batch's tile plan (None: it fails the tile checks,
    or ``tiles`` is off) and whether its largest graph fits the
    single-workgroup pass.  Pure host function."""
    if plan is not None and (tiles == "force" or not fits):
        return "tiles"
    if fits and (plan is not None or not tiles):
        return "fused"
    return "layers"


def _input_grad_tiles(rq: _Request, c, h: BatchHandle, plan, s, e):
    """One ``dr_ginet_large_input_grad_pass`` (three launches): the batch's rows of ``dx`` in place."""
    if c.dz is None:  # dZ of the largest batch, rows of r4(F) words
        c.dz = torch.empty(max(c.rmax, 1) * (-(-rq.f // 4) * 4), dtype=torch.float32, device=rq.dev)
    p, ig = _input_grad_args(rq, c, h, s, e)
    rc = _lib.load().dr_ginet_large_input_grad_pass(rq.store.cstruct(), h.descs.data_ptr(), h.B, plan.c, rq.w, p, ig, c.dz.data_ptr(), plan.conv_lds, plan.tail_lds, _lib.stream_ptr(rq.dev))
    _lib.check(rc, "dr_ginet_large_input_grad_pass")


def _input_grad_layers(rq: _Request, h: BatchHandle, s, e):
    """The batch through ``layered.ginet_forward`` and ``torch.autograd.grad``."""
    t = copy.copy(layered.batch_tensors(h))
    rq.out[s:e], g = _layer_grad(rq.model, t, t.x.detach().clone(), rq.seed_t[s:e], pred=rq.target == "pred")
    rq.write_rows(s, e, g)


def input_gradients(model, dataset, indices=None, batch_size=64, target=None, seed=None, fused=None, *, tiles=None, dx_out=None, _large=None) -> InputGradients:
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

    ``tiles`` (default ``TILES_DEFAULT``): the route of graphs beyond one
    workgroup's LDS.  ``False``: the layer route.  ``True``: a batch that
    passes the tile checks — an fp32 store, ``fused`` not off, no non-finite
    graph, at most 64 depth-0 clusters per graph, the tile plan within one
    workgroup's LDS — runs ``dr_ginet_large_input_grad_pass`` (all of its
    graphs together, ``path`` ``"tiles"``) when its largest graph does not fit
    the single-workgroup pass, and that pass when it does; a batch that fails
    the checks takes the layer route.  ``"force"``: every batch that passes the
    checks takes the tile route (a diagnostic: the two fused routes write equal
    bits).

    One ``dx`` buffer ``[rows, x_stride]`` serves the whole call: every launch
    writes its graphs' rows in place (``dr_input_grad.row_off``); the scratch
    slab and head of the training pass are allocated once.  The gradient with
    respect to ``edge_attr`` is exactly zero (module docstring) and is not
    returned."""
    _check_target("input_gradients", model, target, seed)
    tiles = _check_tiles(tiles)
    rq = _Request("input_gradients", model, dataset, indices, batch_size, target, seed, fused, dx_out, "dx_out")
    # each graph's first row of dx; the fused routes' slab and head (the training pass's partials: scratch here) and the tile route's dZ, made on their first batch
    c = SimpleNamespace(row_off=torch.from_numpy(rq.node_off[:-1].copy()).to(rq.dev) if rq.n else None, slab=None, head=None, dz=None)
    c.rmax = max((int(rq.node_off[e] - rq.node_off[s]) for s, e in rq.batches), default=0)
    for s, e in rq.batches:
        h = rq.handle(s, e)
        if _large is not None:  # (the tests' knob: the plan's tile size and forms)
            h.large_tile, h.large_halos, h.large_atomic_max = _large["tile"], _large["halos"], _large["atomic_max"]
        z = agg_x_for(ginet.SPEC, h) if rq.kernel_ok else None  # (the Z array off: the kernel's gather form, z null and zs 0)
        zs = rq.store.agg_x_stride if z is not None else 0
        plan = _tile_plan(rq, h) if tiles else None
        fits = rq.kernel_ok and not h.nonfinite and _lds("dr_ginet_input_grad_lds_bytes", h, rq.out_dim, zs) <= LDS_MAX
        route = _route(tiles, plan, fits)
        if route == "tiles":
            _input_grad_tiles(rq, c, h, plan, s, e)
        elif route == "fused":
            _input_grad_fused(rq, c, h, s, e, z, zs)
        else:
            _input_grad_layers(rq, h, s, e)
        rq.taken.add(route)
    return InputGradients(rq.view, rq.out, rq.seed_t, rq.node_off, rq.idx, rq.path())


# ---------------------------------------------------------------------------
# Integrated gradients
# ---------------------------------------------------------------------------

# Workgroups per graph of dr_ginet_integrated_grad_pass when ``groups`` is not
# given: the fastest of {1, 2, 4, 8, 32} at 32 steps on a batch of 64 (DESIGN §5,
# profiles/integrated_gradients/bench_ig.txt); capped by the step count, never
# by the batch, so a graph gets the same bits alone and inside a batch.
IG_GROUPS_DEFAULT = 4

# The same for dr_ginet_large_integrated_grad_pass (the tile route), where a
# group is a row of the grid of every launch: the fastest of {1, 2, 4, 8, 32} at
# 32 steps on a batch of 8 atom-level graphs (DESIGN §5 "Integrated gradients
# on tiles", profiles/integrated_gradients_large/bench_ig_large.txt: more
# groups shorten the rounds but ig_finish_kernel, one workgroup per graph,
# reads every group's rows); capped by the step count, never by the batch.
IG_TILE_GROUPS_DEFAULT = 2

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
class IntegratedGradients(_NodeRows):
    attr: torch.Tensor  # [rows, F] device view: (x - baseline) * sum_s w_s g_s, the requested graphs' nodes in order
    out: torch.Tensor  # [n, out_dim] eval-mode outputs at x
    out_baseline: torch.Tensor  # [n, out_dim] eval-mode outputs at the baseline
    seed: torch.Tensor  # [n, out_dim] the upstream gradient each graph was seeded with
    attr_sum: torch.Tensor  # [n] fp64: each graph's sum of attr
    delta: torch.Tensor  # [n] fp64: attr_sum - (out - out_baseline) . seed, the completeness gap (quadrature error)
    node_off: np.ndarray  # host int64 [n + 1]: graph i's rows are node_off[i] .. node_off[i + 1] - 1
    indices: np.ndarray  # host int64 [n]: the graphs' positions in the store
    path: str  # "fused", "tiles", "layers" or "mixed" (more than one route)
    alpha: np.ndarray  # host fp32 [steps]: the quadrature nodes the device used
    weight: np.ndarray  # host fp32 [steps]: the quadrature weights the device used

    @property
    def dx(self):
        """``attr`` under the name ``node_scores`` / ``top_nodes`` read."""
        return self.attr

    def node_attr(self):
        """The signed attribution of each node, ``[rows]``: its features' sum."""
        return self.attr.sum(dim=1)


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


def _group_scratch(rq: _Request, c, n_groups):
    """Per-group slab / head / out of the training pass and the partial rows of a fused route: scratch, made on the route's first batch."""
    f, out_dim, dev = rq.f, rq.out_dim, rq.dev
    return SimpleNamespace(
        n_groups=n_groups,
        slab=torch.empty(n_groups * rq.bmax * ginet.slab_stride(f), dtype=torch.float32, device=dev),
        head=torch.zeros(n_groups * rq.bmax * ginet.head_stride(out_dim), dtype=torch.float32, device=dev),
        outs=torch.empty(n_groups * rq.bmax * out_dim, dtype=torch.float32, device=dev),
        part=torch.empty((n_groups, max(c.rmax, 1), rq.xs), dtype=torch.float32, device=dev),
    )


def _baseline_out_and_seed(rq: _Request, c, s, e):
    """After the forward at ``x`` (and at a given baseline): a zero baseline's outputs in closed form, and the ``"pred"`` seed."""
    if c.xb is None:
        if c.out_b0 is None:  # a zero baseline's outputs: Z = 0 pools to zero features, so the head on a zero vector
            c.out_b0 = torch.relu(rq.params[13]) @ rq.params[14].t() + rq.params[15]
        c.out_b[s:e] = c.out_b0
    if rq.target == "pred":
        rq.seed_t[s:e] = _one_hot_pred(rq.out[s:e])


def _integrated_args(rq: _Request, c, g, s, e):
    """What the two fused routes hand their entry alike: the seeded pass and the ``dr_integrated_grad`` of the batch's rows, on the group scratch ``g``."""
    p = make_pass(rq.out_dim, _lib.DR_PASS_FORWARD | _lib.DR_PASS_BACKWARD, dout=rq.seed_t[s:e])
    ig = _lib.IntegratedGradC()
    ig.attr, ig.row_off, ig.dx_stride = rq.buf.data_ptr(), c.offs.data_ptr() + 8 * s, rq.xs
    ig.n_steps, ig.n_groups = c.n_steps, g.n_groups
    ig.alpha, ig.weight = c.quad_t.data_ptr(), c.quad_t.data_ptr() + 4 * c.n_steps
    ig.zb, ig.xb = _lib.ptr(c.zb), _lib.ptr(c.xb) if c.zb is not None else None
    ig.part, ig.part_off, ig.part_rows = g.part.data_ptr(), c.offs.data_ptr() + 8 * (rq.n + s), g.part.shape[1]
    ig.attr_sum = c.attr_sum.data_ptr() + 8 * s
    ig.slab, ig.head, ig.out = g.slab.data_ptr(), g.head.data_ptr(), g.outs.data_ptr()
    return p, ig


def _integrated_fused(rq: _Request, c, h: BatchHandle, s, e):
    """The Z-input forward at ``x``, the same at the baseline, and one
    ``dr_ginet_integrated_grad_pass``: the batch's rows of ``attr`` in place."""
    out_dim, dev, zs = rq.out_dim, rq.dev, c.zs
    if c.fused is None:
        c.fused = _group_scratch(rq, c, c.n_groups)
    _forward_z(h, rq.w, out_dim, c.z_all, zs, rq.out[s:e])
    if c.zb is not None:
        _forward_z(h, rq.w, out_dim, c.zb, zs, c.out_b[s:e])
    _baseline_out_and_seed(rq, c, s, e)
    p, ig = _integrated_args(rq, c, c.fused, s, e)
    lds = _lds("dr_ginet_integrated_grad_lds_bytes", h, out_dim, zs)
    rc = _lib.load().dr_ginet_integrated_grad_pass(rq.store.cstruct(), h.descs.data_ptr(), h.B, rq.w, p, ig, c.z_all.data_ptr(), zs, lds, _lib.stream_ptr(dev))
    _lib.check(rc, "dr_ginet_integrated_grad_pass")


def _integrated_tiles(rq: _Request, c, h: BatchHandle, plan, s, e):
    """The large-graph forward at ``x``, the same at the baseline (the store
    struct with ``x`` pointing at it), and one
    ``dr_ginet_large_integrated_grad_pass``: the batch's rows of ``attr`` in place."""
    out_dim, dev, lib = rq.out_dim, rq.dev, _lib.load()
    t = c.tiles
    if t is None:  # the groups' scratch and workspaces for the largest batch, made on the first tile batch
        c.tiles = t = _group_scratch(rq, c, c.n_groups_tiles)
        rows, g = max(c.rmax, 1), t.n_groups
        t.dz = torch.empty(g * rows * (-(-rq.f // 4) * 4), dtype=torch.float32, device=dev)
        t.z = torch.empty(g * rows * rq.xs, dtype=torch.float32, device=dev)
        t.keys = torch.zeros(g * rq.bmax * K0_TILES_MAX * 32, dtype=torch.int64, device=dev)  # zero between passes, as LargePlan's
        t.part_val = t.part_arg = None
    if not plan.c.part_key and (t.part_val is None or t.part_val.numel() < t.n_groups * plan.n_tiles * plan.k0_max * 32):
        t.part_val = torch.empty(t.n_groups * plan.n_tiles * plan.k0_max * 32, dtype=torch.float32, device=dev)
        t.part_arg = torch.empty(t.n_groups * plan.n_tiles * plan.k0_max * 32, dtype=torch.int32, device=dev)

    def forward(store_c, out):
        p = make_pass(out_dim, _lib.DR_PASS_FORWARD, out=out)
        _lib.check(lib.dr_ginet_large_pass(store_c, h.descs.data_ptr(), h.B, plan.c, rq.w, p, plan.conv_lds, plan.tail_lds, _lib.stream_ptr(dev)), "dr_ginet_large_pass")

    forward(rq.store.cstruct(), rq.out[s:e])
    if c.xb is not None:
        forward(c.store_b, c.out_b[s:e])
    _baseline_out_and_seed(rq, c, s, e)
    p, ig = _integrated_args(rq, c, t, s, e)
    ws = _lib.IgTilesC()
    ws.dz, ws.z, ws.rows, ws.zb_stride = t.dz.data_ptr(), t.z.data_ptr(), max(c.rmax, 1), c.zs
    ws.part_key, ws.part_val, ws.part_arg = t.keys.data_ptr(), _lib.ptr(t.part_val), _lib.ptr(t.part_arg)
    rc = lib.dr_ginet_large_integrated_grad_pass(rq.store.cstruct(), h.descs.data_ptr(), h.B, plan.c, rq.w, p, ig, ws, plan.conv_lds, plan.tail_lds, _lib.stream_ptr(dev))
    _lib.check(rc, "dr_ginet_large_integrated_grad_pass")


def _integrated_layers(rq: _Request, c, h: BatchHandle, s, e):
    """The batch step by step: :func:`_layer_grad` at every quadrature node."""
    t = copy.copy(layered.batch_tensors(h))
    x0 = t.x.detach()
    b0 = torch.zeros_like(x0) if c.xb is None else c.xb[_store_rows(rq.store, rq.idx[s:e], rq.dev), : rq.f]
    with torch.no_grad():
        o = layered.ginet_forward(rq.model, t, training=False)
        t.x = b0
        c.out_b[s:e] = layered.ginet_forward(rq.model, t, training=False)
    rq.out[s:e] = o
    if rq.target == "pred":
        rq.seed_t[s:e] = _one_hot_pred(o)
    acc = torch.zeros_like(x0)
    for k in range(c.n_steps):
        _, g = _layer_grad(rq.model, t, b0 + float(c.alpha[k]) * (x0 - b0), rq.seed_t[s:e])
        acc += float(c.weight[k]) * g
    a = (x0 - b0) * acc
    rq.write_rows(s, e, a)
    c.attr_sum[s:e] = torch.zeros(e - s, dtype=torch.float64, device=rq.dev).index_add_(0, t.batch.long(), a.double().sum(dim=1))


def integrated_gradients(model, dataset, indices=None, batch_size=64, target=None, seed=None, baseline=None, steps=32, method="gausslegendre", groups=None, fused=None, *, tiles=None, attr_out=None, _quadrature=None, _large=None) -> IntegratedGradients:
    """Integrated gradients (Sundararajan et al. 2017) of ``out . seed`` with
    respect to the node features, for the graphs ``indices`` of ``dataset``:

        attr[i, f] = (x[i, f] - b[i, f]) * sum_s w_s g_s[i, f],
        g_s = d (out(x_s) . seed) / dx  at  x_s = b + alpha_s (x - b),

    with ``(alpha, w) = quadrature(method, steps)`` rounded to fp32.  The
    attributions of a graph sum to ``(out - out_baseline) . seed`` up to the
    quadrature's error, which ``delta`` reports per graph.

    ``model``, ``dataset``, ``indices``, ``batch_size``, ``target``, ``seed``,
    ``fused``, ``tiles``: as :func:`input_gradients` (``"pred"`` is decided
    once, from the forward at ``x``).  ``baseline``: ``None`` (zeros: the dataset mean of
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
    and is not returned.

    ``tiles`` (default ``TILES_DEFAULT``, off): with ``True``, a batch that
    passes :func:`input_gradients`' tile checks runs
    ``dr_ginet_large_integrated_grad_pass`` (``path`` ``"tiles"``) when
    ``dr_ginet_integrated_grad_lds_bytes`` of its largest graph exceeds one
    workgroup's LDS, and the single-workgroup pass when it does not; a batch
    that fails the checks takes the layer route.  ``"force"``: every batch
    that passes the checks takes the tile route (the two fused routes write
    equal bits at equal ``groups``).  There ``out`` and ``out_baseline`` come
    from forward ``dr_ginet_large_pass`` launches (a zero baseline: the closed
    form), and ``groups`` defaults to ``IG_TILE_GROUPS_DEFAULT`` (at most
    ``steps``): a group is a row of the grid of each of the ``2 R + 2`` launches,
    ``R = ceil(steps / groups)``.  The tile plan is built once per batch; the
    groups' workspaces are allocated once per call for the largest batch, per
    group about ``rows * (x_stride + r4(F) + x_stride) * 4`` bytes (its Z rows,
    its running ``dZ`` and its partial ``attr`` rows; ``rows``: the batch's
    nodes) plus 16 KiB of pooling keys per graph, beside the slab / head
    scratch every fused route has."""
    _check_target("integrated_gradients", model, target, seed)
    tiles = _check_tiles(tiles)
    alpha, weight, n_groups = _check_ig_args(model, steps, method, groups, baseline, _quadrature)
    rq = _Request("integrated_gradients", model, dataset, indices, batch_size, target, seed, fused, attr_out, "attr_out")
    # once per call: the baseline in x's layout (xb) and its neighbour sums in Z's (zb), the buffers beside the request's, the offsets and the quadrature on the device
    store, dev, f, n, node_off, batches = rq.store, rq.dev, rq.f, rq.n, rq.node_off, rq.batches
    c = SimpleNamespace(alpha=alpha, weight=weight, n_steps=int(alpha.size), n_groups=n_groups, xb=None, zb=None, out_b0=None, fused=None, tiles=None, store_b=None)
    c.n_groups_tiles = n_groups if groups is not None else min(IG_TILE_GROUPS_DEFAULT, c.n_steps)
    c.z_all = store.agg_x() if rq.kernel_ok else None  # None: there is no gather form, every batch takes the layer route
    c.zs = store.agg_x_stride
    if baseline is not None:
        b_t = torch.as_tensor(baseline, dtype=torch.float32, device=dev)
        c.xb = xb = torch.zeros((max(1, int(store.x.shape[0])), rq.xs), dtype=torch.float32, device=dev)
        if b_t.dim() == 1:
            xb[:, :f] = b_t
        else:
            if b_t.shape[0] != rq.rows:
                msg = f"baseline must be [{f}] or [{rq.rows}, {f}] (got {list(b_t.shape)})"
                raise ValueError(msg)
            if np.unique(rq.idx).size != rq.idx.size:
                msg = "a per-node baseline needs every requested graph named once"
                raise ValueError(msg)
            xb[_store_rows(store, rq.idx, dev), :f] = b_t
        if c.z_all is not None or (tiles and rq.kernel_ok):  # (the tile route gathers Z itself and reads only zb)
            c.zb = torch.empty((xb.shape[0], c.zs), dtype=torch.float32, device=dev)  # Z's layout
            c.store_b = st = _lib.GraphStoreC.from_buffer_copy(store.cstruct())  # the store at the baseline
            st.x = xb.data_ptr()
            _lib.check(_lib.load().dr_aggregate_x(st, c.zb.data_ptr(), c.zs, 0, store.n_graphs, _lib.stream_ptr(dev)), "dr_aggregate_x")
    c.out_b = torch.empty(n, rq.out_dim, dtype=torch.float32, device=dev)
    c.attr_sum = torch.zeros(n, dtype=torch.float64, device=dev)
    c.rmax = max((int(node_off[e] - node_off[s]) for s, e in batches), default=0)
    c.offs = None  # [2, n]: each graph's first row of attr, and its first row inside its batch (the partial rows)
    if n:
        first = np.repeat(node_off[[s for s, _ in batches]], [e - s for s, e in batches])
        c.offs = torch.from_numpy(np.stack([node_off[:-1], node_off[:-1] - first])).to(dev)
    c.quad_t = torch.from_numpy(np.stack([alpha, weight])).to(dev)  # [2, S]
    for s, e in batches:
        h = rq.handle(s, e)
        if _large is not None:  # (the tests' knob: the plan's tile size and forms)
            h.large_tile, h.large_halos, h.large_atomic_max = _large["tile"], _large["halos"], _large["atomic_max"]
        lds = _lds("dr_ginet_integrated_grad_lds_bytes", h, rq.out_dim, c.zs) if c.z_all is not None else -1
        fits = c.z_all is not None and not h.nonfinite and 0 <= lds <= LDS_MAX
        plan = _tile_plan(rq, h) if tiles else None
        route = _route(tiles, plan, fits)
        if route == "tiles":
            _integrated_tiles(rq, c, h, plan, s, e)
        elif route == "fused":
            _integrated_fused(rq, c, h, s, e)
        else:
            _integrated_layers(rq, c, h, s, e)
        rq.taken.add(route)
    delta = c.attr_sum - ((rq.out.double() - c.out_b.double()) * rq.seed_t.double()).sum(dim=1)
    return IntegratedGradients(rq.view, rq.out, c.out_b, rq.seed_t, c.attr_sum, delta, rq.node_off, rq.idx, rq.path(), alpha, weight)


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
    store = store_of(store_or_dataset, dx.device)
    x = store.x[_store_rows(store, result.indices, dx.device), : dx.shape[1]]
    return (x * dx).sum(dim=1)


def top_nodes(result: InputGradients, scores, i, k):
    """Host indices (local node ids, int64) of the ``k`` highest-scoring nodes
    of the i-th requested graph, highest first; equal scores in node order."""
    s = scores[result.rows(i)].detach().cpu().numpy()
    return np.argsort(-s, kind="stable")[: max(0, int(k))].astype(np.int64)
