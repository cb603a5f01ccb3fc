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

The forward side: ``FusedEnsembleForward`` runs the members' eval-mode passes
over their batches as grids (max B_k, K) of forward-only rows of the same
``dr_ginet_multi_pass``, one launch per step, the whole run captured into one
HIP graph.  ``train_ensemble`` validates through it; ``predict_ensemble`` adds
the ensemble's mean and spread (``dr_ensemble_stats``, one launch);
``out_of_fold_predictions`` gives a cross-validation's out-of-fold scores.

Scores formed on the device: a runner built with a ``ScoreSpec`` ends its run
(its captured graph) with one ``dr_ensemble_score`` launch, which turns the
predictions, the staged graph ids and the store's targets into K rows of fp64
sums in a fixed order; ``scores_from_sums`` makes the loss over the whole
held-out set and the metrics (RMSE, MAE, Pearson r, R^2; accuracy, the
confusion matrix and its binary rates) of them on the host.
``train_ensemble(val_loss="device")`` validates that way, ``patience`` /
``restore_best`` stop members early on the validation loss
(``MemberStopping``), and ``score_ensemble`` scores the members and the
ensemble's mean prediction.
"""

from __future__ import annotations

import contextlib
import ctypes
from collections.abc import Sequence
from dataclasses import dataclass

import numpy as np
import torch

from deeprank2_amd import _lib, layered
from deeprank2_amd.engine import LOSS_KINDS, OPT_KINDS, FusedTrainStep
from deeprank2_amd.epoch import StagedBatches, store_fits
from deeprank2_amd.fused import LDS_MAX, BatchHandle, agg_x_for, capture_after_warmup, launch, lds_for, make_pass, slab_rows_for, z_lds_for
from deeprank2_amd.neuralnets.gnn.ginet import GINet
from deeprank2_amd.store import store_of

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
        models = _check_members(models, "an ensemble step")
        k = len(models)
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
            g = capture_after_warmup(lambda: self.step(handles, dropout=dropout), self.device)
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
    val_path: str | None = None  # "fused" or "sequential": how the held-out graphs were evaluated (None without val_indices)
    val_scores: list | None = None  # val_loss="device": the epochs' ``Scores`` of the held-out sets, one per epoch run
    best_epoch: np.ndarray | None = None  # [K] int: the epoch of each member's lowest validation loss (-1: none; None without val_indices)
    stopped_epoch: np.ndarray | None = None  # [K] int: the epoch after which patience stopped the member (-1: never)
    step: FusedEnsembleStep | None = None  # the step that trained them: ``step.steps[k]`` holds member k's optimizer state and device counters


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


def _weighted_mean_loss(step: FusedTrainStep, triples):
    """The step's loss over the batches ``triples`` yields as (out, y, len):
    each batch's fp32 torch loss times its length, summed in float64 on the
    device (one ``.item()``), over the graph count; NaN without a graph."""
    total = torch.zeros((), dtype=torch.float64, device=step.device)
    count = 0
    with torch.no_grad():
        for out, y, n in triples:
            total += _mean_loss(step, out, y).double() * n
            count += n
    return float(total.item()) / count if count else float("nan")


def _held_out_loss(step: FusedTrainStep, store, indices, batch_size):
    """Member's loss over ``indices`` through its forward-only pass (eval mode: no dropout)."""
    model = step.model
    was_training = model.training
    model.eval()

    def triples():  # (run from inside the helper's no_grad)
        for idx in epoch_batches(indices, batch_size, False, 0, 0, 0):
            y = torch.from_numpy(np.asarray(store.packed.y)[idx]).to(step.device, torch.float32)
            yield model(_Handle(BatchHandle(store, idx.astype(np.int32)))), y, len(idx)

    try:
        return _weighted_mean_loss(step, triples())
    finally:
        model.train(was_training)


def _check_members(models, what):
    """The refusals every multi-member runner makes before any device work."""
    models = list(models)
    k = len(models)
    if not 1 <= k <= MAX_MEMBERS:
        msg = f"{what} takes 1 to {MAX_MEMBERS} members (got {k})"
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
    return models


def _check_batches(sizes, batches, n_graphs=None):
    """``batches[k][s]`` as int64 arrays of graph ids, checked against the
    batch sizes ``sizes[k][s]`` a runner was built for (and, with ``n_graphs``,
    against the store's range).  Host only."""
    if len(batches) != len(sizes):
        msg = f"{len(sizes)} members, {len(batches)} lists of batches"
        raise ValueError(msg)
    out = []
    for k, (want, given) in enumerate(zip(sizes, batches)):
        arrs = [np.asarray(b, dtype=np.int64).reshape(-1) for b in given]
        if [a.size for a in arrs] != list(want):
            msg = f"member {k}: batches of sizes {[a.size for a in arrs]} do not match the runner's batch sizes {list(want)}"
            raise ValueError(msg)
        if n_graphs is not None and any(a.size and (a.min() < 0 or a.max() >= n_graphs) for a in arrs):
            msg = f"member {k}: a graph id lies outside the store's 0..{n_graphs - 1}"
            raise ValueError(msg)
        out.append(arrs)
    return out


SCORE_SUMS = _lib.DR_SCORE_SUMS


@dataclass
class ScoreSpec:
    """What a ``FusedEnsembleForward`` scores its predictions with
    (``dr_ensemble_score`` as the run's last launch): the loss of the training
    step (a key of ``LOSS_KINDS``), SmoothL1's beta / Huber's delta (default
    1.0), the cross entropy's class weights, and whether the confusion matrix
    is counted (cross entropy only)."""

    loss: str
    loss_param: float | None = None
    class_weights: object = None
    confusion: bool = False

    def checked(self, out_dim):
        """The spec with its defaults filled in, refused on the host as the C entry would."""
        if self.loss not in LOSS_KINDS:
            msg = f"loss must be one of {sorted(LOSS_KINDS)} (got {self.loss!r})"
            raise ValueError(msg)
        param = float(1.0 if self.loss_param is None else self.loss_param) if self.loss in ("smooth_l1", "huber") else 0.0
        if not (param >= 0.0 and param != float("inf")) or (self.loss == "huber" and param == 0.0):
            msg = f"loss_param must be a finite beta >= 0 (smooth_l1) or delta > 0 (huber) (got {self.loss_param!r})"
            raise ValueError(msg)
        if self.loss == "ce" and out_dim < 2:
            msg = "the cross entropy needs at least two outputs"
            raise ValueError(msg)
        if self.loss != "ce" and self.confusion:
            msg = "a confusion matrix is counted for the cross entropy only"
            raise ValueError(msg)
        return ScoreSpec(self.loss, param, self.class_weights if self.loss == "ce" else None, bool(self.confusion))

    @property
    def task(self):
        return "classif" if self.loss == "ce" else "regress"


class _ScoreLaunch:
    """One ``dr_ensemble_score`` over fixed buffers: ``out`` [K, rows, out_dim]
    against ``y[gids]`` (``gids`` [K, rows] or [rows] int64, or None: ``y[i]``),
    member k's first ``n[k]`` rows.  The output buffers are made here (or
    taken); calling the object makes the launch, nothing else, so it can be
    captured."""

    def __init__(self, out, y, gids, n, spec: ScoreSpec, probs, sums=None, confusion=None):
        _lib.require_device(out, y, gids)
        if out.dim() != 3 or out.dtype != torch.float32 or out.stride(2) != 1 or out.stride(1) != out.shape[2]:
            msg = "out must be fp32 [K, n, out] with contiguous [n, out] blocks"
            raise ValueError(msg)
        k, rows, out_dim = out.shape
        spec = spec.checked(out_dim)
        if probs and spec.loss != "ce":
            msg = "probs goes with the cross entropy only"
            raise ValueError(msg)
        if y.dim() != 1 or y.dtype != torch.float32 or not y.is_contiguous():
            msg = "y must be a contiguous fp32 vector (the store's targets)"
            raise ValueError(msg)
        n = [rows] * k if n is None else [int(v) for v in n]
        if len(n) != k or any(v < 0 or v > rows for v in n):
            msg = f"n needs one row count in 0..{rows} per member ({k})"
            raise ValueError(msg)
        gid_stride = 0
        if gids is not None:
            if gids.dtype != torch.int64 or gids.dim() not in (1, 2) or gids.stride(-1) != 1 or gids.shape[-1] < max(n):
                msg = "gids must be int64 [n] or [K, n] with contiguous rows of at least max(n) ids"
                raise ValueError(msg)
            if gids.dim() == 2:
                if gids.shape[0] != k:
                    msg = f"gids has {gids.shape[0]} rows for {k} members"
                    raise ValueError(msg)
                gid_stride = gids.stride(0) if k > 1 else 0
        elif max(n) > y.numel():
            msg = "without gids row i scores against y[i]: more rows than targets"
            raise ValueError(msg)
        cw = spec.class_weights
        if cw is not None:
            cw = torch.as_tensor(cw, dtype=torch.float32, device=out.device).contiguous()
            if cw.numel() != out_dim:
                msg = f"class_weights needs {out_dim} entries (got {cw.numel()})"
                raise ValueError(msg)
        self.out, self.y, self.gids, self.n, self.spec, self.class_w = out, y, gids, n, spec, cw
        self.gid_stride = gid_stride
        self.flags = _lib.DR_SCORE_PROBS if probs else 0
        self._n = (ctypes.c_int32 * k)(*n)
        dev = out.device
        with torch.cuda.device(dev):
            self.sums = torch.zeros(k, SCORE_SUMS, dtype=torch.float64, device=dev) if sums is None else sums
            self.confusion = (torch.zeros(k, out_dim, out_dim, dtype=torch.int64, device=dev) if confusion is None else confusion) if spec.confusion else None

    def __call__(self):
        k, _, out_dim = self.out.shape
        rc = _lib.load().dr_ensemble_score(self.out.data_ptr(), self.out.stride(0), _lib.ptr(self.gids), self.gid_stride, self.y.data_ptr(), self.y.numel(), self._n, k, out_dim,
                                           LOSS_KINDS[self.spec.loss], self.spec.loss_param, _lib.ptr(self.class_w), self.flags, self.sums.data_ptr(), _lib.ptr(self.confusion),
                                           _lib.stream_ptr(self.out.device))  # fmt: skip
        _lib.check(rc, "dr_ensemble_score")


def ensemble_score(out, y, *, gids=None, n=None, loss, loss_param=None, class_weights=None, probs=False, confusion=False):
    """``dr_ensemble_score`` on ``out`` [K, rows, out] (fp32, on the device; a
    view whose members are more than rows * out floats apart is fine; [rows,
    out] is one member) against the targets ``y`` (fp32 device vector, the
    store's ``y``): member k's row i scores against ``y[gids[k, i]]`` (``gids``
    int64 on the device, [K, rows], or [rows] for all members), or ``y[i]``
    without ``gids``; ``n[k]`` (default: all) rows of member k are scored.
    ``loss``: a key of ``LOSS_KINDS``; ``probs``: ``out`` holds probabilities
    (cross entropy: the term is -log p_y).  Returns ``(sums [K, 12] float64 on
    the device, confusion [K, out, out] int64 or None)``; ``scores_from_sums``
    turns them into metrics on the host."""
    if out.dim() == 2:
        out = out.unsqueeze(0)
    launch_ = _ScoreLaunch(out, y, gids, n, ScoreSpec(loss, loss_param, class_weights, confusion), probs)
    with torch.cuda.device(out.device):
        launch_()
    return launch_.sums, launch_.confusion


@dataclass
class Scores:
    """Per-member metrics (arrays [K]) from the sums of ``dr_ensemble_score``;
    a field that does not apply to the task is None."""

    loss: np.ndarray  # the loss over the whole scored set: slot 0 / slot 1 (NaN when slot 1 is 0)
    n: np.ndarray  # rows scored (int64)
    n_nan: np.ndarray  # of those, rows with a NaN term (regression) or a NaN logit (classification)
    n_skipped: np.ndarray  # rows left out: id outside the store, or a target that is no class index
    rmse: np.ndarray | None = None
    mae: np.ndarray | None = None
    pearson: np.ndarray | None = None
    r2: np.ndarray | None = None
    accuracy: np.ndarray | None = None
    confusion: np.ndarray | None = None  # [K, C, C] int64, row = target, column = predicted
    mcc: np.ndarray | None = None
    tpr: np.ndarray | None = None
    tnr: np.ndarray | None = None
    precision: np.ndarray | None = None


def _ratio(num, den):
    """num / den, NaN where den is 0 (or not finite arithmetic: no exception, no warning)."""
    num, den = np.asarray(num, dtype=np.float64), np.asarray(den, dtype=np.float64)
    with np.errstate(all="ignore"):
        return np.where(den == 0, np.nan, num / np.where(den == 0, 1.0, den))


def scores_from_sums(sums, confusion, task):
    """Metrics from ``dr_ensemble_score``'s sums S [K, 12] (numpy, float64) and
    optional confusion matrices [K, C, C]; pure host arithmetic in float64.
    A zero denominator gives NaN.

    Always: ``loss = S0 / S1``, ``n_nan = S2``, ``n_skipped = S3``.

    ``task = "regress"`` (n = S1, d = o - y; S4 = sum d^2, S5 = sum |d|, S6 =
    sum o, S7 = sum y, S8 = sum o^2, S9 = sum y^2, S10 = sum o y)::

        rmse    = sqrt(S4 / n)
        mae     = S5 / n
        pearson = (n S10 - S6 S7) / sqrt((n S8 - S6^2) (n S9 - S7^2))
        r2      = 1 - S4 / (S9 - S7^2 / n)

    ``task = "classif"`` (n = S5, the rows scored; S1 is the sum of the class
    weights): ``accuracy = S4 / n``.  With a confusion matrix M (row = target,
    column = predicted) it is returned, and for two classes, with tn = M00,
    fp = M01, fn = M10, tp = M11::

        tpr       = tp / (tp + fn)
        tnr       = tn / (tn + fp)
        precision = tp / (tp + fp)
        mcc       = (tp tn - fp fn) / sqrt((tp + fp) (tp + fn) (tn + fp) (tn + fn))
    """
    if task not in ENS_KINDS:
        msg = f"task must be one of {sorted(ENS_KINDS)} (got {task!r})"
        raise ValueError(msg)
    s = np.asarray(sums, dtype=np.float64).reshape(-1, SCORE_SUMS)
    loss = _ratio(s[:, 0], s[:, 1])
    n_nan, n_skipped = s[:, 2].astype(np.int64), s[:, 3].astype(np.int64)
    if task == "regress":
        if confusion is not None:
            msg = "a confusion matrix goes with task='classif'"
            raise ValueError(msg)
        n = s[:, 1]
        with np.errstate(all="ignore"):
            rmse = np.sqrt(_ratio(s[:, 4], n))
            pearson = _ratio(n * s[:, 10] - s[:, 6] * s[:, 7], np.sqrt((n * s[:, 8] - s[:, 6] ** 2) * (n * s[:, 9] - s[:, 7] ** 2)))
            r2 = 1.0 - _ratio(s[:, 4], s[:, 9] - _ratio(s[:, 7] ** 2, n))
        return Scores(loss, n.astype(np.int64), n_nan, n_skipped, rmse=rmse, mae=_ratio(s[:, 5], n), pearson=pearson, r2=r2)
    n = s[:, 5]
    res = Scores(loss, n.astype(np.int64), n_nan, n_skipped, accuracy=_ratio(s[:, 4], n))
    if confusion is not None:
        m = np.asarray(confusion, dtype=np.int64)
        m = m.reshape(s.shape[0], m.shape[-2], m.shape[-1])
        res.confusion = m
        if m.shape[-1] == 2:
            tn, fp, fn, tp = (m[:, i, j].astype(np.float64) for i, j in ((0, 0), (0, 1), (1, 0), (1, 1)))
            res.tpr, res.tnr, res.precision = _ratio(tp, tp + fn), _ratio(tn, tn + fp), _ratio(tp, tp + fp)
            with np.errstate(all="ignore"):
                res.mcc = _ratio(tp * tn - fp * fn, np.sqrt((tp + fp) * (tp + fn) * (tn + fp) * (tn + fn)))
    return res


class MemberStopping:
    """The early-stopping bookkeeping of ``train_ensemble``, host only: member
    k's epoch improves when its validation loss falls below its best so far by
    more than ``min_delta`` (the first finite loss always does; a NaN never
    does); after ``patience`` epochs in a row without improvement the member is
    stopped (``patience = None``: never).  ``best_epoch`` / ``stopped_epoch``:
    int arrays [K], -1 for never."""

    def __init__(self, k, patience=None, min_delta=0.0):
        if patience is not None and int(patience) < 1:
            msg = f"patience must be at least 1 (got {patience})"
            raise ValueError(msg)
        if not min_delta >= 0.0:
            msg = f"min_delta must be >= 0 (got {min_delta})"
            raise ValueError(msg)
        self.patience = None if patience is None else int(patience)
        self.min_delta = float(min_delta)
        self.best = np.full(k, np.inf)
        self.best_epoch = np.full(k, -1, dtype=np.int64)
        self.stopped_epoch = np.full(k, -1, dtype=np.int64)
        self.stalled = np.zeros(k, dtype=np.int64)

    @property
    def active(self):
        """[K] bool: the members still training."""
        return self.stopped_epoch < 0

    def update(self, epoch, losses):
        """Enter the epoch's validation losses [K] (a stopped member's entry is
        ignored); returns the members whose best epoch this is."""
        improved = []
        for m, v in enumerate(np.asarray(losses, dtype=np.float64)):
            if self.stopped_epoch[m] >= 0:
                continue
            if v < self.best[m] - self.min_delta:  # (False for NaN)
                self.best[m], self.best_epoch[m], self.stalled[m] = v, epoch, 0
                improved.append(m)
                continue
            self.stalled[m] += 1
            if self.patience is not None and self.stalled[m] >= self.patience:
                self.stopped_epoch[m] = epoch
        return improved


# Whether FusedEnsembleForward runs the multi-member launches by default (the
# measurement behind the choice: DESIGN §5, profiles/ensemble_forward/)
FUSED_FORWARD_DEFAULT = True


class FusedEnsembleForward:
    """The forward passes (eval mode: no dropout, no backward) of K GINet
    members (1 <= K <= 8) over batches of one resident ``GraphStore``.

    ``sizes[k]``: the batch sizes of member k's passes, in order; members may
    have different numbers of batches, and a member without a batch at step s
    sits that step out (``n_batch = 0``).  The runner owns one output buffer
    ``[K, n_max, out_dim]``; ``run(batches)`` (``batches[k][s]``: graph ids
    matching ``sizes``) fills it and returns the views ``[out_k[:n_k]]``.

    Eligible runs (fp32, no non-finite graph in the store, every graph of the
    store inside the per-graph kernel's LDS, no handle with ``force_large`` or
    ``force_layers``) make each step s ONE ``dr_ginet_multi_pass``: a grid
    (max B_k, K) of forward-only rows, Z = A x from the store when it has one,
    LDS sized for the store's largest graph.  After one eager warm-up (Z built,
    LDS attributes set) the whole run is captured into one HIP graph and
    replayed (``captured = False``: the same launches, issued eagerly).
    Otherwise, or with ``fused = False``, each member's batches run in turn
    through the launches ``model(batch)`` makes in eval mode.  Row k of the
    grid runs member k's own launch's code on its arguments, so both paths give
    the same bits.  ``last_path``: "fused" or "sequential".  One exception: a
    batch with non-finite inputs takes the layer path, which sums with torch's
    ``index_add`` (float atomics), so its result equals ``model(batch)`` only up
    to torch's own run-to-run differences unless
    ``torch.use_deterministic_algorithms`` is on.

    ``fused = None`` takes ``FUSED_FORWARD_DEFAULT`` (True, by the measurement
    in DESIGN §5).  ``run`` may be called again without a device sync in
    between: it waits for the previous run's copy of the graph ids before it
    stages the next ones.

    Nothing of a member changes: not its ``training`` flag, parameters,
    optimizer state or device counters (a forward-only pass has no dropout and
    no step counter).  The parameters are read through their device pointers,
    so in-place updates (a training step between two runs) are seen.
    """

    def __init__(self, models, store, sizes, *, fused=None, captured=True, score=None):
        models = _check_members(models, "an ensemble forward")
        if score is not None:
            score = score.checked(models[0].output_shape)
        k = len(models)
        sizes = [[int(b) for b in s] for s in sizes]
        if len(sizes) != k:
            msg = f"sizes has {len(sizes)} entries for {k} members"
            raise ValueError(msg)
        if any(b < 1 for s in sizes for b in s):
            msg = "every batch size must be positive"
            raise ValueError(msg)
        self.params = [m.ordered_params() for m in models]
        devices = {p.device for ps in self.params for p in ps}
        if len(devices) != 1:
            msg = "the members must live on one device"
            raise ValueError(msg)
        if any(not p.is_cuda or not p.is_contiguous() or p.dtype != torch.float32 for ps in self.params for p in ps):
            msg = "FusedEnsembleForward needs contiguous fp32 cuda parameters (no CPU fallback)"
            raise ValueError(msg)
        if store.device != next(iter(devices)):
            msg = f"the members live on {next(iter(devices))}, the store on {store.device}"
            raise ValueError(msg)
        if store.n_feat != models[0].input_shape:
            msg = f"the store has {store.n_feat} node features, the members expect {models[0].input_shape}"
            raise ValueError(msg)
        if not store.packed.has_clusters:
            msg = "GINet pools over the stored clusters: build the dataset with clustering_method set (cluster0/cluster1 are missing)"
            raise ValueError(msg)
        self.models, self.store, self.sizes = models, store, sizes
        self.spec = models[0].fused_spec
        self.out_dim = models[0].output_shape
        self.device = dev = store.device
        self.fused = FUSED_FORWARD_DEFAULT if fused is None else bool(fused)
        self.captured = bool(captured)
        self.last_path = None  # "fused" or "sequential": which the last run() took
        self.graph = None
        self.staged = st = StagedBatches(store, sizes)
        self.handles, self.offs, self.n, self._probe = st.handles, st.offs, st.n, st.probe  # (the probe: the store's largest graph, for LDS and Z)
        with torch.cuda.device(dev):
            self.out = torch.zeros(k, st.n_max, self.out_dim, dtype=torch.float32, device=dev)
        self.score = score
        if score is not None:  # (score = None: no buffer, no launch)
            self._score_launch = _ScoreLaunch(self.out, store.y, st.gids, self.n, score, probs=False)
            self.sums, self.confusion = self._score_launch.sums, self._score_launch.confusion
        self._w = [self.spec.weights(ps) for ps in self.params]
        fwd = _lib.DR_PASS_FORWARD
        self._passes = [[make_pass(self.out_dim, fwd, out=self.out[m, o : o + b]) for o, b in zip(self.offs[m][:-1], sizes[m])] for m in range(k)]
        idle = [make_pass(self.out_dim, fwd, out=self.out[m]) for m in range(k)]  # a member sitting a step out: checked, never read on the device
        self._keep = idle
        self._members = []
        for s in range(st.n_steps):
            arr = (_lib.GinetMemberC * k)()
            for m in range(k):
                if s < len(sizes[m]):
                    h = self.handles[m][s]
                    arr[m].w, arr[m].pass_, arr[m].descs, arr[m].n_batch = ctypes.pointer(self._w[m]), ctypes.pointer(self._passes[m][s]), h.descs.data_ptr(), h.B
                else:
                    arr[m].w, arr[m].pass_, arr[m].descs, arr[m].n_batch = ctypes.pointer(self._w[m]), ctypes.pointer(idle[m]), st.descs.data_ptr(), 0
            self._members.append(arr)

    def views(self):
        """The members' predictions as views of the runner's buffer, ``[out_k[:n_k]]``."""
        return [self.out[m, : self.n[m]] for m in range(len(self.models))]

    def eligible(self) -> bool:
        """The run can take the multi-member launches (``FusedEnsembleStep._fits``
        without the accumulating-pass condition, for the whole store)."""
        if any(h.force_large or h.force_layers for hs in self.handles for h in hs):
            return False
        return store_fits(self.spec, self.store, self.out_dim, self._probe)

    def _launches(self):
        """One dr_ginet_multi_pass per step (nothing is allocated here once Z exists)."""
        lib = _lib.load()
        store = self.store
        z = agg_x_for(self.spec, self._probe)
        lds = z_lds_for(self._probe, self.out_dim) if z is not None else lds_for(self.spec, self._probe, self.out_dim)
        stream = _lib.stream_ptr(self.device)
        for arr in self._members:
            rc = lib.dr_ginet_multi_pass(store.cstruct(), arr, len(self.models), lds, _lib.ptr(z), store.agg_x_stride if z is not None else 0, stream)
            _lib.check(rc, "dr_ginet_multi_pass")
        if self.score is not None:  # the members' sums over the buffer just filled: the run's last launch
            self._score_launch()

    def _sequential(self, batches):
        """Each member's batches in turn, by the launches ``model(batch)`` makes
        in eval mode (``GINet.forward``): the graph pass, or for a batch with
        non-finite inputs the layer path with the attention computed."""
        with torch.no_grad():
            for m, arrs in enumerate(batches):
                for s, ids in enumerate(arrs):
                    h = BatchHandle(self.store, ids.astype(np.int32))
                    h.force_large, h.force_layers = self.handles[m][s].force_large, self.handles[m][s].force_layers
                    if layered.needs_layers(self.spec, h, self.out_dim):
                        o = self.offs[m][s]
                        self.out[m, o : o + h.B].copy_(self.spec.layers(self.models[m], layered.batch_tensors(h), False))
                    else:
                        launch(self.spec, h, self._w[m], self._passes[m][s])
        if self.score is not None:  # the launch the fused path ends with, on the same buffers: the same bits
            self.staged.load(batches)
            self._score_launch()

    def run(self, batches):
        """Predict ``batches[k][s]`` (arrays of graph ids of the store, sizes as
        built) with member k; returns ``[out_k[:n_k]]``, views of the runner's
        buffer that the next ``run`` overwrites."""
        batches = _check_batches(self.sizes, batches, self.store.packed.n_graphs)
        with torch.cuda.device(self.device):
            if self.score is not None and self._score_launch.y is not self.store.y:  # set_targets() since the last run
                self._score_launch = _ScoreLaunch(self.out, self.store.y, self.staged.gids, self.n, self.score, probs=False, sums=self.sums, confusion=self.confusion)
                self.graph = None
            if not (self.fused and self.eligible()):
                self.last_path = "sequential"
                self._sequential(batches)
                return self.views()
            self.last_path = "fused"
            self.staged.load(batches)
            if not self.captured:
                self._launches()
                return self.views()
            if self.graph is None:  # (the warm-up builds Z; a forward changes no state: nothing to put back)
                self.graph = capture_after_warmup(self._launches, self.device)
            self.graph.replay()
        return self.views()


@dataclass
class EnsemblePrediction:
    members: torch.Tensor  # [K, n, out]: every member's predictions (logits for a classifier)
    mean: torch.Tensor  # [n, out]: regression: the members' mean; classification: their mean softmax probability
    spread: torch.Tensor  # regression [n, out]: the unbiased standard deviation over members (NaN for K = 1); classification [n]: the entropy of ``mean``
    label: torch.Tensor | None  # classification [n] int32: arg max of ``mean`` (-1 where it is NaN); None for regression
    indices: np.ndarray  # [n]: the graphs predicted, in order


ENS_KINDS = {"regress": _lib.DR_ENS_REGRESS, "classif": _lib.DR_ENS_CLASSIF}


def ensemble_stats(members, task):
    """``dr_ensemble_stats`` on ``members`` [K, n, out] (fp32, on the device; a
    view whose members are more than n * out floats apart is fine): (mean,
    spread, label) as ``EnsemblePrediction`` holds them."""
    if task not in ENS_KINDS:
        msg = f"task must be one of {sorted(ENS_KINDS)} (got {task!r})"
        raise ValueError(msg)
    _lib.require_device(members)
    k, n, out_dim = members.shape
    if members.dtype != torch.float32 or members.stride(2) != 1 or members.stride(1) != out_dim:
        msg = "members must be fp32 [K, n, out] with contiguous [n, out] blocks"
        raise ValueError(msg)
    dev = members.device
    classif = task == "classif"
    with torch.cuda.device(dev):
        mean = torch.empty(n, out_dim, dtype=torch.float32, device=dev)
        spread = torch.empty((n,) if classif else (n, out_dim), dtype=torch.float32, device=dev)
        label = torch.empty(n, dtype=torch.int32, device=dev) if classif else None
        rc = _lib.load().dr_ensemble_stats(members.data_ptr(), members.stride(0), k, n, out_dim, ENS_KINDS[task], mean.data_ptr(), spread.data_ptr(), _lib.ptr(label), _lib.stream_ptr(dev))
    _lib.check(rc, "dr_ensemble_stats")
    return mean, spread, label


def _device_of(models):
    return next(iter(models[0].parameters())).device


def predict_ensemble(models, dataset, indices=None, batch_size=64, task=None):
    """Score graphs with every member of an ensemble: each member's
    predictions, their mean and their spread (``EnsemblePrediction``; the
    tensors stay on the device).

    Every member predicts the same graphs: ``indices`` (default: all graphs of
    the store), in that order, in batches of ``batch_size`` (the last one may
    be short), through one ``FusedEnsembleForward``; one ``dr_ensemble_stats``
    launch over its buffer then forms the statistics.  ``task``: "regress"
    (mean and unbiased standard deviation) or "classif" (mean softmax
    probability, its entropy, its arg-max label); default "classif" when the
    members have more than one output.

    The runner is kept with the store (``_runner_for``: the last few, with
    their models and buffers, until ``forget_runners(store)``), so predicting
    other graphs in batches of the same sizes replays its captured graph.  The
    returned tensors are the caller's own (``members`` is a copy), and calls may
    follow one another without a device sync.
    """
    models = _check_members(models, "an ensemble prediction")
    if task is None:
        task = "classif" if models[0].output_shape > 1 else "regress"
    if task not in ENS_KINDS:
        msg = f"task must be one of {sorted(ENS_KINDS)} (got {task!r})"
        raise ValueError(msg)
    store = store_of(dataset, _device_of(models))
    idx = np.arange(store.n_graphs, dtype=np.int64) if indices is None else np.asarray(indices, dtype=np.int64).reshape(-1)
    batches = epoch_batches(idx, batch_size, False, 0, 0, 0)
    runner = _runner_for(models, store, [[len(b) for b in batches]] * len(models))
    runner.run([batches] * len(models))
    mean, spread, label = ensemble_stats(runner.out[:, : idx.size], task)  # one launch over the runner's buffer
    return EnsemblePrediction(runner.out[:, : idx.size].clone(), mean, spread, label, idx)


def score_ensemble(models, dataset, indices=None, batch_size=64, loss="mse", loss_param=None, class_weights=None, task=None):
    """Score an ensemble against the store's targets: ``(Scores of the K
    members, Scores of the ensemble, EnsemblePrediction)``.

    ``predict_ensemble`` (its kept runner, its statistics launch) predicts
    ``indices``; then two ``dr_ensemble_score`` launches: the members'
    predictions, and the ensemble's ``mean`` as one more member row (for a
    classifier the mean probability, scored with ``probs``: the loss is
    -log p_y).  ``loss`` and its settings as the training step takes them;
    ``task`` defaults to "classif" for the cross entropy and "regress"
    otherwise and must agree with the loss.  A classifier's scores carry the
    confusion matrix."""
    classif = loss == "ce"
    if task is None:
        task = "classif" if classif else "regress"
    if task not in ENS_KINDS or (task == "classif") != classif:
        msg = f"task {task!r} does not go with loss {loss!r}: 'classif' scores the cross entropy, 'regress' the other losses"
        raise ValueError(msg)
    models = _check_members(models, "an ensemble score")
    store = store_of(dataset, _device_of(models))
    pred = predict_ensemble(models, store, indices, batch_size, task)
    with torch.cuda.device(store.device):
        gids = torch.from_numpy(pred.indices).to(store.device)
    kw = {"gids": gids, "loss": loss, "loss_param": loss_param, "class_weights": class_weights, "confusion": classif}
    m_sums, m_conf = ensemble_score(pred.members, store.y, **kw)
    e_sums, e_conf = ensemble_score(pred.mean.unsqueeze(0), store.y, probs=classif, **kw)
    both = torch.cat([m_sums, e_sums]).cpu().numpy()  # one copy for the K + 1 rows
    conf = None if not classif else torch.cat([m_conf, e_conf]).cpu().numpy()
    k = m_sums.shape[0]
    return (scores_from_sums(both[:k], None if conf is None else conf[:k], task), scores_from_sums(both[k:], None if conf is None else conf[k:], task), pred)


MAX_KEPT_RUNNERS = 4


def forget_runners(store):
    """Drop the forward runners ``predict_ensemble`` keeps with ``store`` (and
    with them their references to the member models, buffers and graphs)."""
    store.__dict__.pop("_dr_ens_forward", None)


def _runner_for(models, store, sizes):
    """The store's ``FusedEnsembleForward`` for these members and batch sizes,
    kept with the store (the last few) so that predicting again replays its
    captured graph; rebuilt when a member's parameters have moved.

    Lifetime: the store then holds up to ``MAX_KEPT_RUNNERS`` runners in
    ``store._dr_ens_forward``, and with each its member models, its
    ``[K, n_max, ...]`` device buffers, its pinned id buffer and its captured
    graph, until the store is dropped or ``forget_runners(store)`` is called.
    A caller who wants the lifetime in hand builds a ``FusedEnsembleForward``
    and calls ``ensemble_stats`` on its buffer."""
    cache = store.__dict__.setdefault("_dr_ens_forward", {})
    key = (tuple(id(m) for m in models), tuple(tuple(int(b) for b in s) for s in sizes))
    r = cache.get(key)
    if r is not None and all(a is b for a, b in zip(r.models, models)) and all(p.data_ptr() == q.data_ptr() for m, ps in zip(models, r.params) for p, q in zip(m.ordered_params(), ps)):
        return r
    r = FusedEnsembleForward(models, store, sizes)
    cache.pop(key, None)
    while len(cache) >= MAX_KEPT_RUNNERS:
        cache.pop(next(iter(cache)))
    cache[key] = r
    return r


class _HeldOut:
    """The members' held-out losses after an epoch: one ``FusedEnsembleForward``
    over every member's ``val_indices`` (built once, run every epoch), then the
    loss ``_held_out_loss`` forms, from the same predictions: the fp32 torch
    loss of each batch's slice, times its length, summed in float64."""

    def __init__(self, ens: FusedEnsembleStep, store, val_indices, batch_size, fused=None, device_loss=False):
        self.steps = ens.steps
        self.batches = [epoch_batches(v, batch_size, False, 0, 0, 0) for v in val_indices]
        st = ens.steps[0]
        self.spec = ScoreSpec(st.loss, st.loss_param, st.class_weights) if device_loss else None
        self.runner = FusedEnsembleForward(ens.models, store, [[len(b) for b in bs] for bs in self.batches], fused=fused, score=self.spec)
        if device_loss:
            return
        y = np.asarray(store.packed.y)
        self.y = [[torch.from_numpy(y[b]).to(ens.device, torch.float32) for b in bs] for bs in self.batches]

    def scores(self):
        """The held-out sets' ``Scores``, formed on the device by the run's last
        launch: one run, one copy of K rows of doubles."""
        self.runner.run(self.batches)
        return scores_from_sums(self.runner.sums.cpu().numpy(), None, self.spec.task)

    def losses(self):
        outs = self.runner.run(self.batches)
        res = []
        for st, out, offs, ys in zip(self.steps, outs, self.runner.offs, self.y):
            res.append(_weighted_mean_loss(st, ((out[o : o + len(y)], y, len(y)) for o, y in zip(offs, ys))))
        return np.array(res)


def _disjoint(val_indices, k):
    """``val_indices`` as K int64 arrays no graph of which is listed twice."""
    if len(val_indices) != k:
        msg = f"val_indices needs one entry per member ({k}, got {len(val_indices)})"
        raise ValueError(msg)
    val = [np.asarray(v, dtype=np.int64).reshape(-1) for v in val_indices]
    flat = np.concatenate(val) if val else np.empty(0, np.int64)
    uniq, counts = np.unique(flat, return_counts=True)
    if (counts > 1).any():
        msg = f"graphs {uniq[counts > 1][:8].tolist()} are held out more than once: out-of-fold predictions need disjoint val_indices"
        raise ValueError(msg)
    return val


def out_of_fold_predictions(models, dataset, val_indices, batch_size=64):
    """The out-of-fold predictions of a cross-validation: ``(pred [G, out]
    float32, member [G] int64)`` over the store's G graphs, row g predicted by
    the member whose ``val_indices`` holds g (a graph no member held out: a
    NaN row and member -1; one held out by two members: ``ValueError``).  The
    members predict their held-out parts together, through one
    ``FusedEnsembleForward``."""
    models = _check_members(models, "an out-of-fold prediction")
    val = _disjoint(val_indices, len(models))
    store = store_of(dataset, _device_of(models))
    dev = store.device
    batches = [epoch_batches(v, batch_size, False, 0, 0, 0) for v in val]
    runner = FusedEnsembleForward(models, store, [[len(b) for b in bs] for bs in batches])
    outs = runner.run(batches)
    with torch.cuda.device(dev):
        pred = torch.full((store.n_graphs, runner.out_dim), float("nan"), dtype=torch.float32, device=dev)
        member = torch.full((store.n_graphs,), -1, dtype=torch.int64, device=dev)
        for m, (v, o) in enumerate(zip(val, outs)):
            if v.size:
                rows = torch.from_numpy(v).to(dev)
                pred.index_copy_(0, rows, o)
                member.index_fill_(0, rows, m)
    return pred, member


def train_ensemble(models, dataset, member_indices=None, nepoch=1, batch_size=32, shuffle=True, seed=0, val_indices=None, val_fused=None,
                   val_loss="host", patience=None, min_delta=0.0, restore_best=False, **step_kw):  # fmt: skip
    """Train the members together over one resident dataset.

    ``dataset``: a ``GraphStore``, a dataset with ``graph_store(device)``, or a
    list of ``GraphRecord``; it is held in HBM once.  ``member_indices[k]``:
    the graphs member k trains on (default: all).  Per epoch member k's batches
    are ``epoch_batches(member_indices[k], batch_size, shuffle, seed, k,
    epoch)``; at step s every member that still has a batch s takes part and
    the others sit out.  ``val_indices[k]`` (optional): member k's held-out
    graphs, evaluated after every epoch through one ``FusedEnsembleForward``
    (``val_fused``: its ``fused``; ``EnsembleResult.val_path`` says which path
    ran), or with ``fused = False`` by each member's own loop.  ``step_kw`` goes to
    ``FusedEnsembleStep``.  Training member k alone with ``FusedTrainStep`` over
    the same batches gives the same parameters and losses, bit for bit.

    ``val_loss``: "host" (the default) forms each member's held-out loss with
    torch from its batches' slices, a float64 sum of fp32 per-batch means;
    "device" has the forward runner end with one ``dr_ensemble_score`` launch,
    so an epoch's validation is one graph replay and one copy of K rows of
    doubles, the loss is the loss over the whole held-out set (sum w l / sum w
    with class weights) whatever ``batch_size`` cut it into, and
    ``EnsembleResult.val_scores`` keeps every epoch's ``Scores``.  The two
    differ in rounding (and, with class weights, in the weighting).

    ``patience`` (needs ``val_indices``): member k stops after ``patience``
    epochs in a row without its validation loss falling by more than
    ``min_delta`` (a NaN loss is no improvement, ``MemberStopping``).  A
    stopped member gets no batches in later epochs, its state stays bit for bit
    as it was, and its ``train_loss`` and ``val_loss`` rows read NaN from then
    on.  ``restore_best``: each member's parameters at its best epoch are kept
    on the device and copied back at the end (the optimizer state stays the
    last epoch's).  ``EnsembleResult.best_epoch`` / ``stopped_epoch`` [K], -1
    for never.
    """
    models = list(models)
    k = len(models)
    if val_loss not in ("host", "device"):
        msg = f"val_loss must be 'host' or 'device' (got {val_loss!r})"
        raise ValueError(msg)
    if val_indices is None and (patience is not None or restore_best or val_loss == "device"):
        msg = "patience, restore_best and val_loss='device' work on the held-out loss: give val_indices"
        raise ValueError(msg)
    stopping = MemberStopping(k, patience, min_delta) if val_indices is not None else None
    step_kw.setdefault("max_batch", batch_size)
    ens = FusedEnsembleStep(models, **step_kw)
    store = store_of(dataset, ens.device)
    if member_indices is None:
        member_indices = [np.arange(store.n_graphs)] * k
    if len(member_indices) != k or (val_indices is not None and len(val_indices) != k):
        msg = f"member_indices / val_indices need one entry per member ({k})"
        raise ValueError(msg)
    train_loss = np.full((nepoch, k), np.nan)
    device_loss = val_loss == "device"
    val_loss = None if val_indices is None else np.full((nepoch, k), np.nan)
    val_scores = [] if device_loss else None
    # the held-out graphs of all members through one forward runner, built once
    # (fused = False: the members' own eval-mode loops, one after another)
    val = _HeldOut(ens, store, val_indices, batch_size, val_fused if ens.fused else False, device_loss) if val_indices is not None and (ens.fused or device_loss) else None
    best = [None] * k  # restore_best: each member's parameters at its best epoch (device copies)
    for epoch in range(nepoch):
        active = np.ones(k, dtype=bool) if stopping is None else stopping.active
        if not active.any():
            break
        batches = [epoch_batches(member_indices[m], batch_size, shuffle, seed, m, epoch) if active[m] else [] for m in range(k)]
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
        if device_loss:
            val_scores.append(val.scores())
            val_loss[epoch] = val_scores[-1].loss
        elif val is not None:
            val_loss[epoch] = val.losses()
        elif val_indices is not None:
            for m in range(k):
                val_loss[epoch, m] = _held_out_loss(ens.steps[m], store, val_indices[m], batch_size)
        if stopping is not None:
            val_loss[epoch, ~active] = np.nan
            for m in stopping.update(epoch, val_loss[epoch]):
                if restore_best:
                    with torch.no_grad():
                        best[m] = [p.detach().clone() for p in models[m].ordered_params()]
    if restore_best:
        with torch.no_grad():
            for m in range(k):
                if best[m] is not None and stopping.best_epoch[m] != epoch:
                    for p, b in zip(models[m].ordered_params(), best[m]):
                        p.copy_(b)
    val_path = None if val_indices is None else "sequential" if val is None else val.runner.last_path
    if stopping is None:
        return EnsembleResult(train_loss, val_loss, models, val_path, step=ens)
    return EnsembleResult(train_loss, val_loss, models, val_path, val_scores, stopping.best_epoch, stopping.stopped_epoch, ens)
