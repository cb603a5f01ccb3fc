"""Several GINet models trained together over one resident dataset: an
ensemble, the folds of a k-fold cross-validation, a few seeds, a small
learning-rate or weight-decay sweep.

One model's step at B = 64 occupies 64 of the device's 256 CUs for the length
of one graph's chain of phases, so K such runs one after another
leave most of the chip idle K times over.  ``FusedEnsembleStep`` steps up to
eight members in the two launches one member takes:

1. ``dr_ginet_multi_pass``: a grid (max B_k, K) whose row k is member k's
   per-graph pass on its own batch, weights, loss and dropout stream;
2. ``dr_reduce_update_multi``: a grid (blocks, K) whose row k is member k's
   gradient reduction and optimizer update with its own hyper-parameters.

Each row runs the code the member's own launch runs, on the same arguments in
the same order, so every member's parameters, optimizer state, loss and outputs
are bit for bit those of training it alone with ``FusedTrainStep``.  The store
(and its Z = A x array) is read once per launch by all members.

``train_ensemble`` is the loop around it; ``kfold_indices`` and
``epoch_batches`` are the pure index helpers it uses.
"""

from __future__ import annotations

import contextlib
import ctypes
from collections.abc import Sequence
from dataclasses import dataclass

import numpy as np
import torch

from deeprank2_amd import _lib
from deeprank2_amd.engine import LOSS_KINDS, OPT_KINDS, FusedTrainStep
from deeprank2_amd.fused import LDS_MAX, BatchHandle, agg_x_for, lds_for, slab_rows_for, z_lds_for
from deeprank2_amd.neuralnets.gnn.ginet import GINet

MAX_MEMBERS = _lib.DR_MAX_MEMBERS


def _per_member(value, k, name, pair=False):
    """``value`` as a list of K settings: a scalar (``pair``: a 2-tuple) for
    all members, or a length-K sequence with one per member (a sweep)."""
    if pair:
        each = isinstance(value, Sequence) and len(value) > 0 and all(isinstance(v, Sequence) for v in value)
    else:
        each = isinstance(value, (Sequence, np.ndarray)) and not isinstance(value, str)
    if not each:
        return [tuple(value) if pair else value] * k
    if len(value) != k:
        msg = f"{name} has {len(value)} entries for {k} members"
        raise ValueError(msg)
    return [tuple(v) if pair else float(v) for v in value]


class FusedEnsembleStep:
    """K independent GINet members (1 <= K <= 8) stepping together.

    Built on K ordinary ``FusedTrainStep`` objects (``.steps``), whose buffers,
    C structs, device counters and optimizer state dicts it uses: a member can
    be stepped alone at any time and its checkpoints are the torch classes'
    own.  ``lr``, ``weight_decay``, ``betas`` and ``eps`` take one value or one
    per member; ``optimizer`` and ``loss`` are shared.  ``fused = False`` makes
    every step run the members' own steps in order (same results).
    """

    def __init__(self, models, *, lr=1e-3, weight_decay=1e-5, betas=(0.9, 0.999), eps=1e-8, optimizer="adam", loss="mse", loss_param=None,
                 class_weights=None, max_batch=64, process_group=None, compute_dtype="f32", fused=True):  # fmt: skip
        models = list(models)
        k = len(models)
        if not 1 <= k <= MAX_MEMBERS:
            msg = f"an ensemble step takes 1 to {MAX_MEMBERS} members (got {k})"
            raise ValueError(msg)
        if any(type(m) is not GINet for m in models):
            msg = f"every member must be a GINet (got {sorted({type(m).__name__ for m in models})})"
            raise ValueError(msg)
        if len({(m.input_shape, m.output_shape) for m in models}) != 1:
            msg = "the members must share input_shape and output_shape"
            raise ValueError(msg)
        if len({id(m) for m in models}) != k:
            msg = "the members must be distinct model objects"
            raise ValueError(msg)
        if process_group is not None:
            msg = "the ensemble step is single-device: train data-parallel members with FusedTrainStep"
            raise ValueError(msg)
        if compute_dtype != "f32":
            msg = f"the ensemble step computes in fp32 (got compute_dtype={compute_dtype!r})"
            raise ValueError(msg)
        if loss not in LOSS_KINDS or optimizer not in OPT_KINDS:
            msg = f"loss must be one of {sorted(LOSS_KINDS)} and optimizer one of {sorted(OPT_KINDS)}"
            raise ValueError(msg)
        lrs, wds = _per_member(lr, k, "lr"), _per_member(weight_decay, k, "weight_decay")
        bts, epss = _per_member(betas, k, "betas", pair=True), _per_member(eps, k, "eps")
        self.models = models
        self.steps = [
            FusedTrainStep(m, lr=lrs[i], weight_decay=wds[i], betas=bts[i], eps=epss[i], loss=loss, class_weights=class_weights, max_batch=max_batch, optimizer=optimizer, loss_param=loss_param)
            for i, m in enumerate(models)
        ]
        self.device = self.steps[0].device
        if any(st.device != self.device for st in self.steps):
            msg = "the members must live on one device"
            raise ValueError(msg)
        self.spec = self.steps[0].spec
        self.out_dim = self.steps[0].out_dim
        self.optimizer = optimizer
        self.fused = bool(fused)
        self.last_path = None  # "fused" or "sequential": which the last step() ran
        # the members' losses side by side: every member's step writes its slot
        # (its own FusedTrainStep.step too); a member sitting a step out keeps its last value
        self.losses = torch.zeros(k, dtype=torch.float32, device=self.device)
        for i, st in enumerate(self.steps):
            st.loss_out = self.losses[i : i + 1]
        self._members = (_lib.GinetMemberC * k)()
        self._reduce_bufs = {}  # (B_k, loss_scale_k) per member -> (device argument buffer, blocks)
        self._reduce_for = None  # the members' structs and buffers those were built from
        self._captured = []  # argument buffers a captured graph reads (never evicted)

    # ---- dispatch ----
    def _fits(self, k, h: BatchHandle) -> bool:
        """Member k's batch can take its row of the two multi-member launches."""
        st = self.steps[k]
        if h.nonfinite or h.force_large or getattr(h, "force_layers", False):
            return False
        if lds_for(self.spec, h, self.out_dim) > LDS_MAX:
            return False
        return st._acc_rows(h) == 0  # noqa: SLF001

    def step(self, handles, dropout=True):
        """One training step of every member k on ``handles[k]`` (batches of
        one shared ``GraphStore``; ``None``: the member sits this step out and
        its state stays bit for bit as it was).  Returns (losses [K] device
        view, [out_k views, None for an absent member])."""
        if len(handles) != len(self.steps):
            msg = f"{len(self.steps)} members, {len(handles)} batches"
            raise ValueError(msg)
        present = [k for k, h in enumerate(handles) if h is not None]
        if not present:
            return self.losses, [None] * len(handles)
        store = handles[present[0]].store
        if any(handles[k].store is not store for k in present):
            msg = "the members' batches must come from one GraphStore"
            raise ValueError(msg)
        if self.fused and all(self._fits(k, handles[k]) for k in present):
            self.last_path = "fused"
            self._fused_step(store, handles, present, dropout)
        else:
            self.last_path = "sequential"
            for k in present:
                self.steps[k].step(handles[k], dropout=dropout)
        return self.losses, [None if h is None else self.steps[k].out[: h.B] for k, h in enumerate(handles)]

    def _fused_step(self, store, handles, present, dropout):
        lib = _lib.load()
        stream = _lib.stream_ptr(self.device)
        first = handles[present[0]]
        z = agg_x_for(self.spec, first)  # (no present batch is non-finite: one answer for the store)
        lds = 0
        key = []
        for k, st in enumerate(self.steps):
            h = handles[k]
            m = self._members[k]
            if h is None:  # an empty row: its structs are checked, never read on the device
                m.w, m.pass_, m.descs, m.n_batch = ctypes.pointer(st._w), ctypes.pointer(st._pass), first.descs.data_ptr(), 0  # noqa: SLF001
                key.append((0, 0.0))
                continue
            st._ensure(h.B)  # noqa: SLF001
            scale = st.loss_scale(h, h.B)
            p = st._pass if (dropout and self.spec.dropout > 0 and st.model.dropout > 0) else st._pass_nodrop  # noqa: SLF001
            p.loss_scale = scale
            m.w, m.pass_, m.descs, m.n_batch = ctypes.pointer(st._w), ctypes.pointer(p), h.descs.data_ptr(), h.B  # noqa: SLF001
            lds = max(lds, z_lds_for(h, self.out_dim) if z is not None else lds_for(self.spec, h, self.out_dim))
            key.append((h.B, float(scale)))
        # the reduce's argument buffer is found (or built and uploaded) before the pass is
        # launched, so a failure leaves no member half stepped
        buf, blocks = self._reduce_args(tuple(key), handles)
        rc = lib.dr_ginet_multi_pass(store.cstruct(), self._members, len(self.steps), lds, _lib.ptr(z), store.agg_x_stride if z is not None else 0, stream)
        _lib.check(rc, "dr_ginet_multi_pass")
        for k in present:
            self.steps[k].step_count += 1
        _lib.check(lib.dr_reduce_update_multi(buf.data_ptr(), len(self.steps), blocks, OPT_KINDS[self.optimizer], stream), "dr_reduce_update_multi")

    MAX_REDUCE_BUFS = 64  # argument buffers kept (within an epoch only the last batch's differs)

    def _reduce_args(self, key, handles):
        """The device argument buffer of ``dr_reduce_update_multi`` for these
        batch sizes and loss factors: built and uploaded once, then kept (the
        launch itself copies nothing, so it can be captured)."""
        made_for = [(st._upd, st._table, st.slab.data_ptr()) for st in self.steps]  # noqa: SLF001
        if self._reduce_for is None or any(a is not c or b is not d or e != f for (a, b, e), (c, d, f) in zip(made_for, self._reduce_for)):
            self._reduce_bufs.clear()  # a member's buffers grew or its optimizer settings were reloaded
            self._reduce_for = made_for
        hit = self._reduce_bufs.get(key)
        capturing = torch.cuda.is_current_stream_capturing()
        if hit is not None:
            if capturing:
                self._captured.append(hit[0])
            return hit
        if capturing:
            msg = "dr_reduce_update_multi's arguments for these batches are not on the device yet: run the step once before capturing it (capture() does)"
            raise RuntimeError(msg)
        lib = _lib.load()
        n = len(self.steps)
        members = (_lib.ReduceMemberC * n)()
        for k, st in enumerate(self.steps):
            h = handles[k]
            m = members[k]
            if h is not None:
                st._table.slab_rows = slab_rows_for(self.spec, h)  # noqa: SLF001
            m.t = ctypes.pointer(st._table)  # noqa: SLF001
            m.slab, m.head, m.loss_per_graph, m.loss_out = st.slab.data_ptr(), st.head.data_ptr(), st.lpg.data_ptr(), st.loss_out.data_ptr()
            m.n_batch, m.loss_scale = key[k]
            m.opt = st._upd  # noqa: SLF001
        nbytes = int(lib.dr_reduce_multi_args_bytes(n))
        host = np.zeros(nbytes, dtype=np.uint8)
        blocks = int(lib.dr_reduce_multi_build(members, n, host.ctypes.data, nbytes))
        if blocks < 0:
            _lib.check(blocks, "dr_reduce_multi_build")
        with torch.cuda.device(self.device):
            buf = torch.from_numpy(host).to(self.device)
        if len(self._reduce_bufs) >= self.MAX_REDUCE_BUFS:
            self._reduce_bufs.pop(next(iter(self._reduce_bufs)))
        self._reduce_bufs[key] = (buf, blocks)
        return buf, blocks

    def capture(self, handles, dropout=True):
        """Capture one ensemble step on ``handles`` into a HIP graph
        (``torch.cuda.CUDAGraph``), as ``FusedTrainStep.capture`` does for one
        model: an eager warm-up step first (Z, the reduce's argument buffer,
        LDS attributes exist before the capture begins), then the capture; the
        training state both changed is rolled back.  Every replay advances each
        present member's dropout offset and optimizer step from its device
        counter."""
        with contextlib.ExitStack() as es:
            for st in self.steps:
                es.enter_context(st._state_kept())  # noqa: SLF001
            losses = self.losses.clone()
            self.step(handles, dropout=dropout)
            torch.cuda.synchronize(self.device)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                self.step(handles, dropout=dropout)
            torch.cuda.synchronize(self.device)
        self.losses.copy_(losses)
        return g


def epoch_batches(indices, batch_size, shuffle, seed, member, epoch):
    """The mini-batches of one member's epoch over ``indices``: shuffled (when
    ``shuffle``) by ``np.random.default_rng([seed, member, epoch])``, then cut
    into consecutive batches of ``batch_size`` (the last one may be short)."""
    idx = np.asarray(indices, dtype=np.int64).reshape(-1)
    if batch_size < 1:
        msg = f"batch_size must be positive (got {batch_size})"
        raise ValueError(msg)
    if shuffle:
        idx = idx[np.random.default_rng([int(seed), int(member), int(epoch)]).permutation(idx.size)]
    return [idx[i : i + batch_size].copy() for i in range(0, idx.size, batch_size)]


def kfold_indices(n, k, seed):
    """K folds of ``range(n)`` as [(train_idx, val_idx)], both ascending: the
    validation parts partition ``range(n)`` and their sizes differ by at most 1."""
    if not 1 <= k <= n:
        msg = f"k must be in 1..n (got k={k}, n={n})"
        raise ValueError(msg)
    perm = np.random.default_rng(int(seed)).permutation(n)
    folds = [np.sort(f) for f in np.array_split(perm, k)]
    return [(np.sort(np.concatenate([f for j, f in enumerate(folds) if j != i] or [np.empty(0, np.int64)])).astype(np.int64), folds[i].astype(np.int64)) for i in range(k)]


@dataclass
class EnsembleResult:
    train_loss: np.ndarray  # [nepoch, K]: each member's epoch loss, sum(loss * B) / count as the Trainer forms it
    val_loss: np.ndarray | None  # [nepoch, K] held-out loss, or None without val_indices
    models: list


def _store_of(dataset, device):
    from deeprank2_amd.store import GraphStore, pack_graphs  # noqa: PLC0415

    if isinstance(dataset, GraphStore):
        return dataset
    if callable(getattr(dataset, "graph_store", None)):
        return dataset.graph_store(device)
    return GraphStore(pack_graphs(list(dataset)), device)


class _Handle:
    """What ``GINet.forward`` needs of a batch: its handle."""

    def __init__(self, h):
        self._dr_handle = h


def _mean_loss(step: FusedTrainStep, out, y):
    """The step's loss (mean reduction) on predictions ``out`` and targets ``y``, by torch."""
    fn = torch.nn.functional
    if step.loss == "ce":
        return fn.cross_entropy(out, y.long(), weight=step.class_weights)
    pred = out.reshape(-1)
    if step.loss == "mse":
        return fn.mse_loss(pred, y)
    if step.loss == "l1" or (step.loss == "smooth_l1" and step.loss_param == 0.0):
        return fn.l1_loss(pred, y)
    if step.loss == "smooth_l1":
        return fn.smooth_l1_loss(pred, y, beta=step.loss_param)
    return fn.huber_loss(pred, y, delta=step.loss_param)


def _held_out_loss(step: FusedTrainStep, store, indices, batch_size):
    """Member's loss over ``indices`` through its forward-only pass (eval mode: no dropout)."""
    model = step.model
    was_training = model.training
    model.eval()
    total = torch.zeros((), dtype=torch.float64, device=step.device)
    count = 0
    try:
        with torch.no_grad():
            for idx in epoch_batches(indices, batch_size, False, 0, 0, 0):
                h = BatchHandle(store, idx.astype(np.int32))
                out = model(_Handle(h))
                y = torch.from_numpy(np.asarray(store.packed.y)[idx]).to(step.device, torch.float32)
                total += _mean_loss(step, out, y).double() * len(idx)
                count += len(idx)
    finally:
        model.train(was_training)
    return float(total.item()) / count if count else float("nan")


def train_ensemble(models, dataset, member_indices=None, nepoch=1, batch_size=32, shuffle=True, seed=0, val_indices=None, **step_kw):
    """Train the members together over one resident dataset.

    ``dataset``: a ``GraphStore``, a dataset with ``graph_store(device)``, or a
    list of ``GraphRecord``; it is held in HBM once.  ``member_indices[k]``:
    the graphs member k trains on (default: all).  Per epoch member k's batches
    are ``epoch_batches(member_indices[k], batch_size, shuffle, seed, k,
    epoch)``; at step s every member that still has a batch s takes part and
    the others sit out.  ``val_indices[k]`` (optional): member k's held-out
    graphs, evaluated after every epoch.  ``step_kw`` goes to
    ``FusedEnsembleStep``.  Training member k alone with ``FusedTrainStep`` over
    the same batches gives the same parameters and losses, bit for bit.
    """
    models = list(models)
    k = len(models)
    step_kw.setdefault("max_batch", batch_size)
    ens = FusedEnsembleStep(models, **step_kw)
    store = _store_of(dataset, ens.device)
    if member_indices is None:
        member_indices = [np.arange(store.n_graphs)] * k
    if len(member_indices) != k or (val_indices is not None and len(val_indices) != k):
        msg = f"member_indices / val_indices need one entry per member ({k})"
        raise ValueError(msg)
    train_loss = np.full((nepoch, k), np.nan)
    val_loss = None if val_indices is None else np.full((nepoch, k), np.nan)
    for epoch in range(nepoch):
        batches = [epoch_batches(member_indices[m], batch_size, shuffle, seed, m, epoch) for m in range(k)]
        loss_sum = torch.zeros(k, dtype=torch.float64, device=ens.device)
        count = np.zeros(k, dtype=np.int64)
        for s in range(max(len(b) for b in batches)):
            handles = [BatchHandle(store, b[s].astype(np.int32)) if s < len(b) else None for b in batches]
            sizes = np.asarray([0 if h is None else h.B for h in handles], dtype=np.float64)
            losses, _ = ens.step(handles)
            w = torch.from_numpy(sizes).to(ens.device)
            loss_sum += torch.where(w > 0, losses.double() * w, torch.zeros_like(w))
            count += sizes.astype(np.int64)
        total = loss_sum.cpu().numpy()
        for m in range(k):
            if count[m]:
                train_loss[epoch, m] = float(total[m]) / int(count[m])
        if val_indices is not None:
            for m in range(k):
                val_loss[epoch, m] = _held_out_loss(ens.steps[m], store, val_indices[m], batch_size)
    return EnsembleResult(train_loss, val_loss, models)
