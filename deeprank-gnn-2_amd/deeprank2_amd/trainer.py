"""Trainer — drop-in for ``deeprank2.trainer.Trainer`` on the MI355X path.

Same constructor, ``configure_optimizers`` / ``set_lossfunction`` /
``train`` / ``test`` surface, epoch-0 evaluation, best-model selection,
early stopping, output exporters and checkpoint keys as the reference
(``deeprank2/trainer.py:31-1004``).

The hot loop (``_epoch``, trainer.py:666-724) runs, for a model with a fused
spec under Adam, AdamW or Adamax and MSELoss / L1Loss / SmoothL1Loss /
HuberLoss (regression) or CrossEntropyLoss with optional class weights
(classification) -- :func:`fused_config` decides --, as two HIP launches per
mini-batch through :class:`~deeprank2_amd.engine.FusedTrainStep` on graphs
already resident in HBM; losses and outputs stay on the device until the
epoch ends (one device->host copy per epoch instead of per-step ``.item()``).
Any other optimizer or loss takes the generic path: the model's autograd
forward/backward (still the HIP graph pass) + the torch optimizer.

Multi-GPU: ``ngpu > 1`` expects one process per GPU started by
``torch.distributed.run`` (``init_process_group`` done by the caller or here
from the environment); each global mini-batch is split across ranks in order
and the gradients are all-reduced once per step.  The reference's
``nn.DataParallel`` (trainer.py:387-389) has no counterpart.

Deliberate differences: the model always runs on the GPU (there is
no CPU path; ``cuda=False`` is accepted and logged); a "best model"
checkpoint is a snapshot (the reference keeps references to live tensors, so
its in-memory best model follows later updates); checkpoints store the
optimizer / loss / dataset types by name so that they load with
``torch.load(weights_only=True)``; ``_precluster`` runs MCL for all graphs
on the GPU and keeps the clusters in memory (the reference rewrites the HDF5
files); Louvain is not recomputed (stored clusters are used).
"""

from __future__ import annotations

import copy
import inspect
import logging
import re
import warnings
from time import time

import numpy as np
import torch
from torch import nn
from torch.nn.functional import softmax

from deeprank2_amd.dataset import CLASSIF, REGRESS, GraphDataset
from deeprank2_amd.distributed import plan_epoch, plan_shards
from deeprank2_amd.epoch import eval_runner_for, runner_for
from deeprank2_amd.engine import FusedTrainStep
from deeprank2_amd.io.checkpoint import load_checkpoint
from deeprank2_amd.exporters import HDF5OutputExporter, OutputExporterCollection
from deeprank2_amd.loader import DataLoader
from deeprank2_amd.utils.earlystopping import EarlyStopping

_log = logging.getLogger(__name__)

regression_losses = (nn.L1Loss, nn.SmoothL1Loss, nn.MSELoss, nn.HuberLoss)
binary_classification_losses = (nn.SoftMarginLoss, nn.BCELoss, nn.BCEWithLogitsLoss)
multi_classification_losses = (nn.CrossEntropyLoss, nn.NLLLoss, nn.PoissonNLLLoss, nn.GaussianNLLLoss, nn.KLDivLoss, nn.MultiLabelMarginLoss, nn.MultiLabelSoftMarginLoss)
other_losses = (nn.HingeEmbeddingLoss, nn.CosineEmbeddingLoss, nn.MarginRankingLoss, nn.TripletMarginLoss, nn.CTCLoss)
classification_losses = multi_classification_losses + binary_classification_losses
classification_tested = (nn.CrossEntropyLoss, nn.NLLLoss, nn.BCELoss, nn.BCEWithLogitsLoss)

_OPTIMIZERS = {c.__name__: c for c in (torch.optim.Adam, torch.optim.AdamW, torch.optim.SGD, torch.optim.RMSprop, torch.optim.Adagrad, torch.optim.Adadelta, torch.optim.Adamax, torch.optim.NAdam, torch.optim.RAdam)}
_LOSSES = {c.__name__: c for c in regression_losses + classification_losses + other_losses}


_FUSED_OPTIMIZERS = {torch.optim.Adam: "adam", torch.optim.AdamW: "adamw", torch.optim.Adamax: "adamax"}
_FUSED_REGRESSION = {nn.MSELoss: ("mse", None), nn.L1Loss: ("l1", None), nn.SmoothL1Loss: ("smooth_l1", "beta"), nn.HuberLoss: ("huber", "delta")}


def fused_config(optimizer, lossfunction, task):
    """What :class:`~deeprank2_amd.engine.FusedTrainStep` is to be built with
    for this torch optimizer and loss instance, when the kernels compute
    exactly that configuration: ``(optimizer kind, {"lr", "weight_decay",
    "betas", "eps"}, loss kind, loss_param, class_weights)``; else ``None``
    (the generic loop runs).  Pure: reads the two objects only.

    Optimizers: exactly ``torch.optim.Adam`` (with
    ``decoupled_weight_decay=True``: the AdamW rule), ``AdamW`` or ``Adamax``,
    one parameter group, a float ``lr``, ``maximize`` and ``amsgrad`` off.
    Losses, ``reduction="mean"``: MSE / L1 / SmoothL1 / Huber for regression,
    CrossEntropyLoss (no label smoothing, default ``ignore_index``) for
    classification."""
    kind = _FUSED_OPTIMIZERS.get(type(optimizer))
    if kind is None or len(optimizer.param_groups) != 1:
        return None
    g = optimizer.param_groups[0]
    if g.get("amsgrad") or g.get("maximize") or not isinstance(g["lr"], float):  # (a tensor lr: the generic loop)
        return None
    if kind == "adam" and g.get("decoupled_weight_decay"):
        kind = "adamw"
    hyper = {"lr": float(g["lr"]), "weight_decay": float(g["weight_decay"]), "betas": tuple(float(b) for b in g["betas"]), "eps": float(g["eps"])}
    lf = lossfunction
    if getattr(lf, "reduction", None) != "mean":
        return None
    if task == REGRESS and type(lf) in _FUSED_REGRESSION:
        loss, attr = _FUSED_REGRESSION[type(lf)]
        return kind, hyper, loss, (float(getattr(lf, attr)) if attr else None), None
    if task == CLASSIF and type(lf) is nn.CrossEntropyLoss and lf.label_smoothing == 0 and lf.ignore_index == -100:  # noqa: PLR2004
        return kind, hyper, "ce", None, lf.weight
    return None


class Trainer:
    # ngpu > 1: how a global batch is spread over the ranks (distributed.plan_shards):
    # "auto" (contiguous unless imbalanced by edges), "contiguous" or "edges"
    shard_policy = "auto"
    # one process, fused step, every graph on the per-graph kernel: each training
    # epoch replays one captured HIP graph of all its steps (epoch.py)
    capture_epochs = True

    def __init__(  # noqa: PLR0913, PLR0912, C901
        self,
        neuralnet: type[nn.Module] | None = None,
        dataset_train: GraphDataset | None = None,
        dataset_val: GraphDataset | None = None,
        dataset_test: GraphDataset | None = None,
        val_size: float | int | None = None,
        test_size: float | int | None = None,
        class_weights: bool = False,
        pretrained_model: str | None = None,
        cuda: bool = False,
        ngpu: int = 0,
        output_exporters: list | None = None,
        precluster: bool = True,
    ):
        self.neuralnet = neuralnet
        self.pretrained_model = pretrained_model
        self._adopt_datasets(dataset_train, dataset_val, dataset_test, val_size, test_size)
        self.cuda = cuda
        self._select_device(ngpu)
        self._init_output_exporters(output_exporters)
        self.data_type = self.batch_size_train = self.batch_size_test = self.shuffle = None
        self.model_load_state_dict = None
        self._fused = None
        self._runners = {}
        if self.pretrained_model is None:
            self._setup_for_training(class_weights, precluster)
        else:
            self._setup_from_pretrained()

    # ------------------------------------------------------------------ setup
    # Every precondition is a (holds, exception type, message) rule, checked in
    # order; the exception types and messages are the reference's (its tests,
    # tests/test_trainer.py:287-656, assert them).
    @staticmethod
    def _enforce(rules):
        for holds, exc, msg in rules:
            if not holds():
                raise exc(msg)

    def _select_device(self, ngpu):
        """The model always runs on the GPU when one is visible; ngpu > 1 means one process per GPU."""
        self.ngpu = ngpu
        self.process_group = None
        if not torch.cuda.is_available():
            self.device = torch.device("cpu")
            _log.warning("No GPU visible: models can be built and inspected but not trained or evaluated (no CPU fallback).")
            return
        self.device = torch.device("cuda", torch.cuda.current_device())
        if not self.cuda:
            _log.info("deeprank2_amd has no CPU path: the model runs on the GPU although cuda=False was given.")
        self.ngpu = max(1, ngpu)
        if self.ngpu > 1:
            self._enforce([(torch.distributed.is_initialized, ValueError, "ngpu > 1 runs one process per GPU: launch with torch.distributed.run (torchrun) and init_process_group first")])
            self.process_group = torch.distributed.group.WORLD

    def _setup_for_training(self, class_weights, precluster):
        self._enforce([
            (lambda: self.dataset_train is not None, ValueError, "No training data specified. Training data is required if there is no pretrained model."),
            (lambda: self.neuralnet is not None, ValueError, "No neural network specified. Specifying a model framework is required if there is no pretrained model."),
        ])  # fmt: skip
        self._init_from_dataset(self.dataset_train)
        self.optimizer = None
        self.class_weights = class_weights
        self.subset = self.dataset_train.subset
        self.epoch_saved_model = None
        self._enforce([(lambda: self.target is not None, ValueError, "No target set. You need to choose a target (set in the dataset) for training.")])
        self._load_model()
        if self.clustering_method is None:
            return
        self._enforce([(lambda: self.clustering_method in ("mcl", "louvain"), ValueError, f"Invalid node clustering method: {self.clustering_method}. Please set clustering_method to 'mcl', 'louvain' or None.")])
        # every dataset the run will read gets the same pre-clustering; a missing
        # validation set is split off the (pre-clustered) training set
        if precluster:
            self._precluster(self.dataset_train)
        if self.dataset_val is None:
            _log.warning("No validation dataset given. Randomly splitting training set in training set and validation set.")
            self.dataset_train, self.dataset_val = _divide_dataset(self.dataset_train, splitsize=self.val_size, process_group=self.process_group)
        elif precluster:
            self._precluster(self.dataset_val)
        if precluster and self.dataset_test is not None:
            self._precluster(self.dataset_test)

    def _setup_from_pretrained(self):
        self._enforce([
            (lambda: self.neuralnet is not None, ValueError, "No neural network class found. Please add it to complete loading the pretrained model."),
            (lambda: self.dataset_test is not None, ValueError, "No dataset_test found. Please add it to evaluate the pretrained model."),
        ])  # fmt: skip
        for attr, name in (("dataset_train", "dataset_train"), ("dataset_val", "dataset_val")):
            if getattr(self, attr) is not None:
                setattr(self, attr, None)
                _log.warning(f"Pretrained model loaded: {name} will be ignored.")
        self._init_from_dataset(self.dataset_test)
        self._load_params()
        self._load_pretrained_model()

    def _init_output_exporters(self, output_exporters):
        self._output_exporters = OutputExporterCollection(*(output_exporters if output_exporters is not None else [HDF5OutputExporter("./output")]))

    def _adopt_datasets(self, dataset_train, dataset_val, dataset_test, val_size, test_size):
        """The three datasets after the consistency rules, with val / test split
        off the training set when only a size is given (a given set wins)."""
        self._check_dataset_equivalence(dataset_train, dataset_val, dataset_test)
        self.dataset_train, self.dataset_val, self.dataset_test = dataset_train, dataset_val, dataset_test
        self.val_size, self.test_size = val_size, test_size
        for size, attr, what, param in ((test_size, "dataset_test", "Test", "test_size"), (val_size, "dataset_val", "Validation", "val_size")):
            if size is None:
                continue
            if getattr(self, attr) is not None:
                _log.warning(f"{what} dataset was provided to Trainer; {param} parameter is ignored.")
                continue
            self.dataset_train, split = _divide_dataset(self.dataset_train, size)
            setattr(self, attr, split)

    def _check_dataset_equivalence(self, dataset_train, dataset_val, dataset_test):
        """valid / test sets must name the training set they standardise by (train_source)."""
        if dataset_train is None:
            self._enforce([(lambda: dataset_test is not None, ValueError, "Please provide at least a train or test dataset")])
            return
        self._enforce([(lambda: isinstance(dataset_train, GraphDataset), TypeError, f"train dataset is not the right type {type(dataset_train)}. Make sure it's a GraphDataset")])
        for ds, kind in ((dataset_val, "valid"), (dataset_test, "test")):
            if ds is not None:
                self._enforce([
                    (lambda ds=ds: ds.train_source is not None, ValueError, f"{kind} dataset has train_source parameter set to None. Make sure to set it as a valid training data source."),
                    (lambda ds=ds: ds.train_source is dataset_train or ds.train_source == dataset_train, ValueError, f"{kind} dataset has different train_source parameter from Trainer. Make sure to assign equivalent train_source in Trainer."),
                ])  # fmt: skip

    def _init_from_dataset(self, dataset):
        self._enforce([(lambda: isinstance(dataset, GraphDataset), TypeError, f"Incorrect `dataset` type provided: {type(dataset)}. Please provide a `GraphDataset` object instead.")])
        for attr in ("clustering_method", "node_features", "edge_features", "features_transform", "means", "devs", "target", "target_transform", "task", "classes", "classes_to_index"):
            setattr(self, attr, getattr(dataset, attr))
        self.features = None

    def _load_model(self):
        self._put_model_to_device(self.dataset_train)
        self.configure_optimizers()
        self.set_lossfunction()

    def _precluster(self, dataset):
        """trainer.py:319-348: MCL depth_0 on every graph, depth_1 on the
        pooled graph, for all graphs at once on the GPU (``dr_mcl``).  The
        reference writes the result into the HDF5 files; here it is installed
        in the dataset (``GraphDataset.set_clusters``).  Louvain is not
        provided (randomised; stored clusters are used with a warning)."""
        if self.clustering_method.lower() != "mcl":
            _log.warning(f"{self.clustering_method} clustering is not recomputed by deeprank2_amd: the clusters stored in the HDF5 files are used.")
            return
        if self.device.type != "cuda":
            _log.warning("No GPU visible: MCL pre-clustering skipped, the clusters stored in the HDF5 files are used.")
            return
        from deeprank2_amd import clustering  # noqa: PLC0415

        graphs = []
        for fname, mol in dataset.index_entries:
            a = dataset.graph_arrays(fname, mol)
            graphs.append((a["edge_index"], a["pos"].shape[0]))
        c0, c1 = clustering.precluster_graphs(graphs, self.device)
        dataset.set_clusters({e: (a, b) for e, a, b in zip(dataset.index_entries, c0, c1)})

    def _put_model_to_device(self, dataset):
        if self.task == REGRESS:
            self.output_shape = 1
        elif self.task == CLASSIF:
            self.output_shape = len(self.classes)
        d0 = dataset.get(0)
        target_shape = d0.y.shape[0] if d0.y is not None else None
        self.model = self.neuralnet(d0.num_features, self.output_shape, len(dataset.edge_features)).to(self.device)
        if self.process_group is not None:  # every replica starts from rank 0's initialisation
            src_rank = torch.distributed.get_global_rank(self.process_group, 0)
            with torch.no_grad():
                for t in [*self.model.parameters(), *self.model.buffers()]:
                    torch.distributed.broadcast(t.data, src_rank, group=self.process_group)
        for e in self._output_exporters:
            if not e.is_compatible_with(self.output_shape, target_shape):
                msg = f"Output exporter of type {type(e)}\n\tis not compatible with output shape {self.output_shape}\n\tand target shape {target_shape}."
                raise ValueError(msg)

    def configure_optimizers(self, optimizer=None, lr: float = 0.001, weight_decay: float = 1e-05):
        """trainer.py:401-426.  ``None`` -> Adam.  Adam, AdamW and Adamax run on
        the fused path (:func:`fused_config`); any other optimizer on the generic loop."""
        self.lr = lr
        self.weight_decay = weight_decay
        cls = torch.optim.Adam if optimizer is None else optimizer
        try:
            self.optimizer = cls(self.model.parameters(), lr=lr, weight_decay=weight_decay)
        except Exception as e:
            _log.error(e)
            _log.info("Invalid optimizer. Please use only optimizers classes from torch.optim package.")
            raise
        self._fused = None

    def set_lossfunction(self, lossfunction=None, override_invalid: bool = False):  # noqa: C901
        """trainer.py:428-501 (same validity rules per task)."""

        def invalid():
            text = f"The provided loss function ({lossfunction}) is not appropriate for {self.task} tasks."
            if override_invalid:
                _log.warning(text + " override_invalid is set: training continues with it.")
            else:
                raise ValueError(text + "\n\tIf you want to use this loss function anyway, set override_invalid to True.")

        if lossfunction in other_losses:
            invalid()
            custom = False
        else:
            custom = lossfunction is not None and lossfunction not in (regression_losses + classification_losses)
        if self.task == REGRESS:
            if lossfunction is None:
                lossfunction = nn.MSELoss
            elif custom:
                _log.warning(f"The provided loss function ({lossfunction}) is not part of the default list.")
            elif lossfunction not in regression_losses:
                invalid()
            self.lossfunction = lossfunction()
        elif self.task == CLASSIF:
            if lossfunction is None:
                lossfunction = nn.CrossEntropyLoss
            elif custom:
                _log.warning(f"The provided loss function ({lossfunction}) is not part of the default list.")
            elif lossfunction not in classification_losses:
                invalid()
            self.lossfunction = lossfunction() if not self.class_weights else lossfunction
        self._fused = None

    # --------------------------------------------------------------- helpers
    def _fused_step(self):
        """FusedTrainStep when the configuration is exactly what the kernels compute."""
        if self._fused is not None:
            return self._fused or None
        cfg = fused_config(self.optimizer, self.lossfunction, self.task) if hasattr(self.model, "fused_spec") else None
        if cfg is None or self.output_shape > 16 or self.device.type != "cuda":  # noqa: PLR2004
            self._fused = False
            return None
        kind, hyper, loss, loss_param, w = cfg
        step = FusedTrainStep(self.model, **hyper, loss=loss, loss_param=loss_param, class_weights=w, optimizer=kind, process_group=self.process_group)
        if self.optimizer.state:
            step.load_optimizer_state_dict(self.optimizer.state_dict())
        self._fused = step
        return step

    def _targets_for_kernel(self, dataset, device):
        """The in-kernel CE loss reads a class index per graph: map the stored
        class values through ``classes_to_index`` once per store."""
        store = dataset.graph_store(device)
        if self.task != CLASSIF or getattr(store, "_dr_class_index", None) == self.classes_to_index:
            return store
        y = dataset._targets_of(list(range(len(dataset))))  # noqa: SLF001
        if y is not None:
            store.set_targets(np.array([self.classes_to_index[int(v)] for v in y.tolist()], dtype=np.float32))
            store._dr_class_index = dict(self.classes_to_index)  # noqa: SLF001
        return store

    def _shard(self, ds, idx):
        """This rank's share of the global batch ``idx`` and the plan behind it
        (replacing nn.DataParallel's replicate/scatter,
        trainer.py:387-389): contiguous shards in global order, or — when that
        split leaves one rank more than 1.25x the mean edge load, as in a batch
        mixing residue, SRV and atom-level graphs (config 5) — greedy edge
        bin packing; every rank derives the same plan from the edge counts.
        Returns (local positions, plan); (idx, None) without a process group."""
        if self.process_group is None:
            return np.asarray(idx), None
        pg = self.process_group  # the group's own rank / size (a subgroup need not start at global rank 0)
        idx = np.asarray(idx)
        plan = plan_shards(ds.edge_counts(idx), torch.distributed.get_world_size(pg), policy=self.shard_policy)
        return idx[plan.positions[torch.distributed.get_rank(pg)]], plan

    def _shard_epoch(self, ds, batches):
        """``_shard`` for every global batch of an epoch (``plan_epoch``: the
        same plans, computed together): [(local positions, plan)]."""
        pg = self.process_group
        idx_all = np.concatenate([np.asarray(b) for b in batches]) if batches else np.zeros(0, np.int64)
        plans = plan_epoch(ds.edge_counts(idx_all), [len(b) for b in batches], torch.distributed.get_world_size(pg), policy=self.shard_policy)
        rank = torch.distributed.get_rank(pg)
        out = []
        for idx, pl in zip(batches, plans):
            pos = pl.positions[rank]
            if pl.balanced:
                out.append((np.asarray(idx)[pos], pl))
            else:  # contiguous: a slice
                lo = int(pos[0]) if len(pos) else 0
                out.append((np.asarray(idx)[lo : lo + len(pos)], pl))
        return out

    def _format_output(self, pred, target=None):
        """trainer.py:807-835."""
        if self.task == CLASSIF and target is not None:
            target = torch.tensor([self.classes_to_index[x] if isinstance(x, str) else self.classes_to_index[int(x)] for x in target])
            if isinstance(self.lossfunction, nn.BCELoss | nn.BCEWithLogitsLoss):
                msg = "BCELoss and BCEWithLogitsLoss are currently not supported."
                raise ValueError(msg)
            if isinstance(self.lossfunction, classification_losses) and not isinstance(self.lossfunction, classification_tested):
                msg = f"{self.lossfunction} is currently not supported.\n\tSupported loss functions for classification: {classification_tested}."
                raise ValueError(msg)
        elif self.task == REGRESS:
            pred = pred.reshape(-1)
        if target is not None:
            target = target.to(self.device)
        return pred, target

    def _export_pred(self, pred):
        return softmax(pred.detach(), dim=1) if self.task == CLASSIF else pred.detach().reshape(-1)

    # ---------------------------------------------------------------- train
    def train(  # noqa: PLR0912, PLR0915, C901
        self,
        nepoch: int = 1,
        batch_size: int = 32,
        shuffle: bool = True,
        earlystop_patience: int | None = None,
        earlystop_maxgap: float | None = None,
        min_epoch: int = 10,
        validate: bool = False,
        num_workers: int = 0,
        best_model: bool = True,
        filename: str | None = "model.pth.tar",
    ):
        """trainer.py:503-664."""
        if self.dataset_train is None:
            msg = "No training dataset provided."
            raise ValueError(msg)
        self.data_type = type(self.dataset_train)
        self.batch_size_train = batch_size
        self.shuffle = shuffle
        pg = self.process_group
        self.train_loader = DataLoader(self.dataset_train, batch_size=batch_size, shuffle=shuffle, num_workers=num_workers, pin_memory=self.cuda, process_group=pg)
        self.valid_loader = DataLoader(self.dataset_val, batch_size=batch_size, shuffle=shuffle, num_workers=num_workers, pin_memory=self.cuda, process_group=pg) if self.dataset_val is not None else None
        if self.valid_loader is None:
            _log.warning("Training data will be used both for learning and model selection, which may lead to overfitting.")

        if self.task == CLASSIF and self.class_weights:
            y = self.dataset_train._targets_of(list(range(len(self.dataset_train))))  # noqa: SLF001
            counts = torch.tensor([float((y == c).sum()) for c in self.classes], dtype=torch.float32)
            self.weights = 1.0 / counts
            self.weights = self.weights / self.weights.sum()
            try:
                self.lossfunction = self.lossfunction(weight=self.weights.to(self.device))
            except TypeError as e:
                msg = f"Loss function {self.lossfunction} does not allow for weighted classes.\n\tPlease use a different loss function or set class_weights to False.\n"
                raise ValueError(msg) from e
            self._fused = None
        else:
            self.weights = None

        # model selection: a checkpoint whenever the monitored loss (validation
        # when validating, else training) equals the lowest so far; without one
        # (best_model False, or NaN losses) the last epoch's model is kept, with
        # the reference's warning whenever no selection happened
        history = {"training": [], "validation": []}
        monitored = "validation" if validate else "training"
        kept = None
        stopper = EarlyStopping(patience=earlystop_patience, maxgap=earlystop_maxgap, min_epoch=min_epoch, trace_func=_log.info) if (earlystop_patience or earlystop_maxgap) else None
        epoch = 0
        with self._output_exporters:
            self.nepoch = nepoch
            self._eval(self.train_loader, 0, "training")
            if validate:
                self._enforce([(lambda: self.valid_loader is not None, ValueError, "No validation dataset provided.")])
                self._eval(self.valid_loader, 0, "validation")
            while epoch < nepoch:
                epoch += 1
                self._set_mode(True)
                history["training"].append(self._epoch(epoch, "training"))
                if validate:
                    history["validation"].append(self._eval(self.valid_loader, epoch, "validation"))
                seen = history[monitored]
                if best_model and min(seen) == seen[-1]:
                    # as trainer.py:628-631: the snapshot first, then the
                    # attribute, so a checkpoint records the previous best epoch
                    kept = (self._save_model(), epoch)
                    self.epoch_saved_model = epoch
                if validate and stopper is not None:
                    stopper(epoch, history["validation"][-1], history["training"][-1])
                    if stopper.early_stop:
                        break
            if kept is None or not best_model:
                if kept is None:
                    warnings.warn("A model has been saved but the validation and/or the training losses were NaN;\n\ttry to increase the cutoff distance during the data processing or the number of data points during the training.", stacklevel=2)
                kept = (self._save_model(), epoch)
        checkpoint_model, self.epoch_saved_model = kept
        if filename:
            torch.save(checkpoint_model, filename)
        self.opt_loaded_state_dict = checkpoint_model["optimizer_state"]
        self.model_load_state_dict = checkpoint_model["model_state"]
        self.optimizer.load_state_dict(self.opt_loaded_state_dict)
        self.model.load_state_dict(self.model_load_state_dict)
        if self._fused:
            self._fused.load_optimizer_state_dict(self.opt_loaded_state_dict)

    def _epoch(self, epoch_number: int, pass_name: str):
        """trainer.py:666-724: one pass over the training loader."""
        step = self._fused_step()
        t0 = time()
        dev = self.device
        outputs, targets, names = [], [], []
        loss_sum = torch.zeros((), dtype=torch.float64, device=dev)
        count = 0
        ds = self.dataset_train
        batches = self.train_loader.batches()
        if step is not None and self.capture_epochs:
            store = self._targets_for_kernel(ds, dev)
            plans = None
            if self.process_group is None:
                runner = runner_for(step, store, [len(b) for b in batches], self._runners)
            else:  # this rank's shards of the epoch's global batches (every rank plans the same)
                plans = self._shard_epoch(ds, batches)
                # eligibility from the plans, which every rank computes alike: a
                # global batch leaving ANY rank an empty shard sends every rank
                # to the loop, so the ranks' collective sequences stay matched
                if all(min(pl.sizes()) >= 1 for _, pl in plans):
                    runner = runner_for(step, store, [len(lo) for lo, _ in plans], self._runners, global_sizes=[len(b) for b in batches])
                else:
                    runner = None
            if runner is not None:  # the whole epoch as one captured HIP graph (epoch.py)
                return self._epoch_captured(runner, ds, batches, epoch_number, pass_name, t0, plans)
        for idx in batches:
            b = len(idx)
            if step is not None:
                local, plan = self._shard(ds, idx)
                if len(local):
                    loss, out = step.step(ds.batch_handle(local, dev), global_batch=b)
                else:  # global batch smaller than the world
                    loss, out = step.step_empty()
                loss_sum += loss[0].double() * b
                pred = out.clone()
                if self.process_group is not None:
                    pred = _gather_rows(pred, plan, self.process_group)
                pred, y = self._format_output(pred, ds._targets_of(idx))  # noqa: SLF001
            elif self.process_group is not None:
                pred, y, loss = self._generic_ddp_step(ds, idx)
                loss_sum += loss.double() * b
            else:
                batch = ds.batch(idx).to(dev)
                self.optimizer.zero_grad()
                pred = self.model(batch)
                pred, y = self._format_output(pred, batch.y)
                loss = self.lossfunction(pred, y)
                loss.backward()
                self.optimizer.step()
                loss_sum += loss.detach().double() * b
            count += b
            outputs.append(self._export_pred(pred))
            targets.append(y.detach())
            names += [ds.index_entries[i][1] for i in idx]
        epoch_loss = float(loss_sum.item()) / count if count else None
        if step is not None:
            step.check_faults()  # a skipped step (hand-off gave up) is an error, once per epoch
        out_l = torch.cat(outputs).cpu().numpy().tolist() if outputs else []
        tgt_l = torch.cat(targets).cpu().numpy().tolist() if targets else []
        dt = time() - t0
        self._output_exporters.process(pass_name, epoch_number, names, out_l, tgt_l, epoch_loss)
        _log.info(f"{pass_name} loss {epoch_loss} | time {dt}")
        return epoch_loss

    def _epoch_captured(self, runner, ds, batches, epoch_number, pass_name, t0, plans=None):
        """The epoch's fused steps replayed from one HIP graph: the same
        launches, losses and outputs as the per-batch loop (bit for bit), the
        loss sum in the loop's order.  Data parallel (``plans``: this rank's
        shard of each global batch): the per-step loss terms are summed over
        the ranks and the predictions gathered back into global batch order,
        once per epoch.

        Host work overlaps the replay: the device work is queued first (the
        replay, then the exported predictions and the loss terms into one
        buffer), the exporters' names and targets are built from host copies
        while it runs, and ONE device->host copy ends the epoch."""
        if plans is None:
            losses, pred = runner.run(batches)
        else:
            # one collective per epoch: every rank's loss terms travel with its
            # predictions, and the ranks' terms are summed in rank order
            losses, pred = runner.run([lo for lo, _ in plans])
            pred, losses = _gather_epoch_rows(pred, [pl for _, pl in plans], self.process_group, extra=losses)
        nb = len(runner.sizes)
        exp = self._export_pred(self._format_output(pred)[0])
        both = torch.cat([losses.reshape(-1), exp.reshape(-1)])
        # (while the GPU runs the epoch)
        idx_all = np.concatenate([np.asarray(b) for b in batches])
        names = ds.entry_names(idx_all)
        tgt_l = self._host_targets(ds, idx_all).tolist()
        host = both.cpu()
        step_losses = host[:nb].double().numpy()
        loss_sum = 0.0
        # each (rank-summed) step loss is the GLOBAL batch's mean: weight it by
        # the global batch size, as the loop weights loss[0] by len(idx)
        for lv, b in zip(step_losses, runner.global_sizes):
            loss_sum += float(lv) * b
        count = int(idx_all.size)
        epoch_loss = loss_sum / count if count else None
        self._fused.check_faults()
        out_l = host[nb:].view(exp.shape).numpy().tolist()
        dt = time() - t0
        self._output_exporters.process(pass_name, epoch_number, names, out_l, tgt_l, epoch_loss)
        _log.info(f"{pass_name} loss {epoch_loss} | time {dt}")
        return epoch_loss

    def _set_mode(self, training: bool):
        """``model.train(training)`` (trainer.py:667 / :735 switch it per epoch
        and evaluation): the ``training`` flag of every submodule, set directly
        on a module list built once per model (nn.Module.train walks the tree
        through __setattr__, ~40 us per switch for GINet)."""
        mods = getattr(self, "_mode_modules", None)
        if mods is None or mods[0] is not self.model:
            mods = self._mode_modules = (self.model, list(self.model.modules()))
        if type(self.model).train is not nn.Module.train:  # a model with its own train(): keep its semantics
            self.model.train(training)
            return
        for m in mods[1]:
            object.__setattr__(m, "training", training)

    def _host_targets(self, ds, idx):
        """The targets of dataset positions ``idx`` as ``_format_output`` gives
        them (regression: the float values; classification: class indices),
        from a host array built once per dataset; None without targets."""
        y = ds.targets_host()
        if y is None:
            return None
        if self.task != CLASSIF:
            return y[np.asarray(idx, dtype=np.int64)]
        cached = getattr(ds, "_dr_class_targets", None)
        if cached is None or cached[0] != self.classes_to_index:
            cached = (dict(self.classes_to_index), np.array([self.classes_to_index[int(v)] for v in y.tolist()], dtype=np.int64))
            ds._dr_class_targets = cached  # noqa: SLF001
        return cached[1][np.asarray(idx, dtype=np.int64)]

    def _eval_losses(self, pred, y, sizes):
        """Per-batch losses of an evaluation (trainer.py:760-763:
        ``lossfunction(pred, y)`` per mini-batch) from all its predictions at
        once: MSELoss and CrossEntropyLoss (mean, optional class weights) in
        float64 on host copies, with one device->host copy for the whole
        evaluation; any other loss per batch on the device.  Returns the float
        loss of each batch."""
        lf = self.lossfunction
        offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        sizes_a = np.asarray(sizes, dtype=np.float64)
        if isinstance(lf, nn.MSELoss) and lf.reduction == "mean" and self.task != CLASSIF:
            p = pred.reshape(-1).astype(np.float64)
            sq = (p - y.astype(np.float64)) ** 2
            return (np.add.reduceat(sq, offs[:-1]) / sizes_a).tolist() if sq.size else []
        if isinstance(lf, nn.CrossEntropyLoss) and lf.reduction == "mean" and lf.label_smoothing == 0.0 and self.task == CLASSIF and not (y == lf.ignore_index).any():
            z = pred.astype(np.float64)
            m = z.max(1, keepdims=True)
            lse = (m[:, 0] + np.log(np.exp(z - m).sum(1)))
            nll = lse - z[np.arange(z.shape[0]), y]
            w = np.ones(z.shape[0]) if lf.weight is None else lf.weight.detach().cpu().double().numpy()[y]
            return (np.add.reduceat(nll * w, offs[:-1]) / np.add.reduceat(w, offs[:-1])).tolist() if nll.size else []
        dev = self.device
        pt = torch.as_tensor(pred, device=dev)
        yt = torch.as_tensor(y, device=dev)
        return [float(lf(pt[a:b].reshape(-1) if self.task != CLASSIF else pt[a:b], yt[a:b])) for a, b in zip(offs[:-1], offs[1:])]

    def _generic_ddp_step(self, ds, idx):
        """Any optimizer / loss outside the fused step, one process per GPU:
        each rank runs the model on its contiguous shard, its mean loss is
        weighted by the shard's share of the batch (graph count, or the
        class-weight sum for a weighted CrossEntropyLoss), the gradients and
        that loss are SUM-all-reduced in one flat buffer, then every rank
        takes the same optimizer step.  Returns the global predictions,
        targets and loss."""
        pg = self.process_group
        local, plan = self._shard(ds, idx)
        self.optimizer.zero_grad()
        if len(local):
            batch = ds.batch(local).to(self.device)
            pred = self.model(batch)
            pred_l, y_l = self._format_output(pred, batch.y)
        else:  # a global batch smaller than the world: this rank contributes zeros
            pred = torch.zeros((0, self.output_shape), dtype=torch.float32, device=self.device)
            pred_l = y_l = None
        y_all = ds._targets_of(idx)  # noqa: SLF001
        w = getattr(self.lossfunction, "weight", None)
        if w is not None and self.task == CLASSIF:
            cls = torch.tensor([self.classes_to_index[int(v)] for v in y_all.tolist()])
            wh = w.detach().cpu()
            total = float(wh[cls].sum())  # the weighted mean's denominator over the global batch
            local_pos = plan.positions[torch.distributed.get_rank(pg)]
            frac = float(wh[cls[torch.as_tensor(local_pos, dtype=torch.long)]].sum()) / total if total else 0.0
        else:
            frac = len(local) / len(idx)
        if len(local):
            loss = self.lossfunction(pred_l, y_l) * frac
            loss.backward()
        else:
            loss = torch.zeros((), dtype=torch.float32, device=self.device)
        params = [p for p in self.model.parameters() if p.requires_grad]
        flat = torch.cat([*(p.grad.reshape(-1) if p.grad is not None else torch.zeros(p.numel(), device=p.device) for p in params), loss.detach().reshape(1)])
        torch.distributed.all_reduce(flat, group=pg)
        off = 0
        for p in params:
            n = p.numel()
            if p.grad is None:
                p.grad = torch.zeros_like(p)
            p.grad.copy_(flat[off:off + n].view_as(p))
            off += n
        self.optimizer.step()
        pred_all = _gather_rows(pred.detach().contiguous(), plan, pg)
        pred_all, y = self._format_output(pred_all, y_all)
        return pred_all, y, flat[-1]

    def _eval(self, loader: DataLoader, epoch_number: int, pass_name: str):
        """trainer.py:726-795: forward passes, then the per-batch losses and
        the exporters.  The forward passes are one captured HIP graph where the
        model allows it (epoch.EvalRunner), else one launch per batch; either
        way the predictions of the whole evaluation come back in one
        device->host copy and the per-batch losses are computed from them
        (``_eval_losses``), while names and targets come from host arrays."""
        self._set_mode(False)
        dev = self.device
        t0 = time()
        batches = loader.batches()
        ds = loader.dataset
        runner = None
        if self.capture_epochs and getattr(self.model, "fused_spec", None) is not None and self.cuda:
            # the evaluation's forward passes as one captured HIP graph (epoch.EvalRunner)
            runner = eval_runner_for(self.model, self._targets_for_kernel(ds, dev), [len(b) for b in batches], self._runners)
        sizes = [len(b) for b in batches]
        with torch.no_grad():
            if runner is not None:
                pred_all = runner.run(batches)
            elif batches:
                pred_all = torch.cat([self.model(ds.batch(idx).to(dev)) for idx in batches])
            else:
                pred_all = torch.zeros((0, self.output_shape), dtype=torch.float32, device=dev)
            exp = self._export_pred(self._format_output(pred_all)[0])
            both = torch.cat([pred_all.reshape(-1), exp.reshape(-1)])
        # (while the GPU runs the passes)
        idx_all = np.concatenate([np.asarray(b) for b in batches]) if batches else np.zeros(0, np.int64)
        names = ds.entry_names(idx_all)
        y = self._host_targets(ds, idx_all)
        if self.task == CLASSIF and y is not None:
            self._format_output(pred_all[:0], torch.zeros(0))  # the reference's loss-type checks
        host = both.cpu().numpy()
        n_pred = pred_all.numel()
        out_l = host[n_pred:].reshape(exp.shape).tolist()
        if y is not None and len(idx_all):
            loss_sum, count = 0.0, 0
            for lb, n in zip(self._eval_losses(host[:n_pred].reshape(pred_all.shape), y, sizes), sizes):
                loss_sum += lb * n
                count += n
            eval_loss = loss_sum / count
            tgt_l = y.tolist()
        else:
            eval_loss = None
            tgt_l = [None] * len(out_l)
        dt = time() - t0
        self._output_exporters.process(pass_name, epoch_number, names, out_l, tgt_l, eval_loss)
        _log.info(f"{pass_name} loss {eval_loss} | time {dt}")
        self._set_mode(True)
        return eval_loss

    def test(self, batch_size: int = 32, num_workers: int = 0):
        """trainer.py:837-871."""
        if (not self.pretrained_model) and (not self.model_load_state_dict):
            msg = "No pretrained model provided and no training performed. Please provide a pretrained model or train the model before testing."
            raise ValueError(msg)
        self.batch_size_test = batch_size
        if self.dataset_test is None:
            msg = "No test dataset provided."
            raise ValueError(msg)
        self.test_loader = DataLoader(self.dataset_test, batch_size=batch_size, num_workers=num_workers, pin_memory=self.cuda)
        with self._output_exporters:
            self._eval(self.test_loader, self.epoch_saved_model, "testing")

    # ------------------------------------------------------------ checkpoints
    def _optimizer_state(self):
        if self._fused:
            return self._fused.optimizer_state_dict()
        return self.optimizer.state_dict()

    def _save_model(self):
        """trainer.py:910-956, with types stored by name (weights_only-loadable)
        and tensors snapshotted."""
        ft = copy.deepcopy(self.features_transform)
        if ft:
            for v in ft.values():
                if v.get("transform") is None or isinstance(v["transform"], str):
                    continue
                src = inspect.getsource(v["transform"])
                m = re.search(r"[\"|\']transform[\"|\']:.*(lambda.*).*,.*[\"|\']standardize[\"|\'].*", src)
                v["transform"] = m.group(1) if m else None
        lf = self.lossfunction
        return {
            "data_type": "GraphDataset",
            "model_state": {k: t.detach().clone() for k, t in self.model.state_dict().items()},
            "optimizer": type(self.optimizer).__name__,
            "optimizer_state": copy.deepcopy(self._optimizer_state()),
            "lossfunction": (lf if isinstance(lf, type) else type(lf)).__name__,
            "target": self.target,
            "target_transform": self.target_transform,
            "task": self.task,
            "classes": self.classes,
            "classes_to_index": self.classes_to_index,
            "class_weights": self.class_weights,
            "batch_size_train": self.batch_size_train,
            "batch_size_test": self.batch_size_test,
            "val_size": self.val_size,
            "test_size": self.test_size,
            "lr": self.lr,
            "weight_decay": self.weight_decay,
            "epoch_saved_model": self.epoch_saved_model,
            "subset": self.subset,
            "shuffle": self.shuffle,
            "clustering_method": self.clustering_method,
            "node_features": self.node_features,
            "edge_features": self.edge_features,
            "features": self.features,
            "features_transform": ft,
            "means": self.means,
            "devs": self.devs,
            "cuda": self.cuda,
            "ngpu": self.ngpu,
        }

    def _load_params(self):
        """trainer.py:873-908 (weights_only load, or the inert reader for reference checkpoints)."""
        state = load_checkpoint(self.pretrained_model)
        self.data_type = GraphDataset
        self.model_load_state_dict = state["model_state"]
        opt = state["optimizer"]
        self.optimizer = _OPTIMIZERS[opt] if isinstance(opt, str) else type(opt)
        self.opt_loaded_state_dict = state["optimizer_state"]
        lf = state["lossfunction"]
        self.lossfunction = _LOSSES[lf]() if isinstance(lf, str) else lf
        for k in ("target", "target_transform", "task", "classes", "classes_to_index", "class_weights", "batch_size_train", "batch_size_test", "val_size", "test_size", "lr", "weight_decay", "epoch_saved_model", "subset", "shuffle", "clustering_method", "node_features", "edge_features", "features", "features_transform", "means", "devs", "cuda", "ngpu"):
            setattr(self, k, state[k])
        if torch.cuda.is_available():
            self.ngpu = max(1, self.ngpu if self.process_group is not None else 1)

    def _load_pretrained_model(self):
        self.test_loader = DataLoader(self.dataset_test, pin_memory=self.cuda)
        self._put_model_to_device(self.dataset_test)
        self.optimizer = self.optimizer(self.model.parameters(), lr=self.lr, weight_decay=self.weight_decay)
        self.optimizer.load_state_dict(self.opt_loaded_state_dict)
        self.model.load_state_dict(self.model_load_state_dict)


def _gather_rows(local, plan, pg):
    """All ranks' [b_r, out] predictions, put back in global-batch order by the
    shard plan's permutation (the exporters see the reference's row order)."""
    sizes = plan.sizes()
    top = max(sizes)
    # padded to the largest shard: gloo's all_gather takes equal sizes only
    pad = torch.zeros(top, local.shape[1], dtype=local.dtype, device=local.device)
    pad[: local.shape[0]] = local
    bufs = [torch.empty_like(pad) for _ in sizes]
    torch.distributed.all_gather(bufs, pad, group=pg)
    rows = torch.cat([buf[:s] for buf, s in zip(bufs, sizes)])
    if plan.balanced:
        rows = rows[torch.as_tensor(plan.perm, dtype=torch.long, device=rows.device)]
    return rows


def _gather_epoch_rows(local, plans, pg, extra=None):
    """``_gather_rows`` for a whole epoch at once: ``local`` holds this rank's
    rows of every batch, batch after batch; one all-gather (padded to the
    largest rank) and one index gather put every batch's rows back in its
    global order, batch after batch.  ``extra`` (optional, [n] floats: the
    epoch's per-step loss terms) travels in the same all-gather and comes back
    summed over the ranks in rank order: returns (rows, summed extra).  No
    host synchronisation (the index goes up from pinned memory)."""
    world = torch.distributed.get_world_size(pg)
    per_rank = np.array([pl.sizes() for pl in plans], dtype=np.int64).reshape(len(plans), world)  # [batch, rank]
    offs = np.concatenate([np.zeros((1, world), np.int64), np.cumsum(per_rank, 0)])  # each rank's row offset of each batch
    top = int(offs[-1].max()) if len(plans) else 0
    rows_n = max(top, 1)
    # segments batch-major, rank-minor: batch k's rows from rank r start at
    # r * rows_n + offs[k, r]; balanced batches then take their plan's permutation
    lens = per_rank.reshape(-1)
    base = (np.arange(world, dtype=np.int64)[None, :] * rows_n + offs[:-1]).reshape(-1)
    seg0 = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    index = np.repeat(base - seg0, lens) + np.arange(int(lens.sum()), dtype=np.int64)
    b0 = 0
    for k, pl in enumerate(plans):
        b1 = b0 + int(per_rank[k].sum())
        if pl.balanced:
            index[b0:b1] = index[b0:b1][pl.perm]
        b0 = b1
    index_t = torch.from_numpy(index)
    if local.is_cuda:
        index_t = index_t.pin_memory().to(local.device, non_blocking=True)
    c = local.shape[1]
    nx = 0 if extra is None else int(extra.numel())
    flat = torch.zeros(rows_n * c + nx, dtype=local.dtype, device=local.device)
    flat[: local.numel()] = local.reshape(-1)
    if nx:
        flat[rows_n * c :] = extra.reshape(-1)
    bufs = [torch.empty_like(flat) for _ in range(world)]
    torch.distributed.all_gather(bufs, flat, group=pg)
    summed = None
    if nx:
        summed = bufs[0][rows_n * c :].clone()
        for r in range(1, world):
            summed += bufs[r][rows_n * c :]
    rows = torch.cat([bf[: rows_n * c].view(rows_n, c) for bf in bufs])
    out = rows[index_t]
    return out if extra is None else (out, summed)


def _divide_dataset(dataset, splitsize=None, process_group=None):
    """trainer.py:961-1004: random split into (main, split).  With a process
    group every rank takes rank 0's split."""
    if splitsize is None:
        splitsize = 0.25
    full = len(dataset)
    if isinstance(splitsize, float):
        n_split = int(splitsize * full)
    elif isinstance(splitsize, int):
        n_split = splitsize
    else:
        msg = f"type(splitsize) must be float, int or None ({type(splitsize)} detected.)"
        raise TypeError(msg)
    if n_split >= full or n_split < 0:
        msg = f"Invalid Split size: {n_split}.\nSplit size must be a float between 0 and 1 OR an int smaller than the size of the dataset ({full} datapoints)"
        raise ValueError(msg)
    if splitsize == 0:
        return dataset, None
    idx = np.arange(full)
    np.random.default_rng().shuffle(idx)
    if process_group is not None and torch.distributed.get_world_size(process_group) > 1:
        box = [idx]
        torch.distributed.broadcast_object_list(box, src=torch.distributed.get_global_rank(process_group, 0), group=process_group)
        idx = np.asarray(box[0])
    return dataset.subset_entries(idx[n_split:]), dataset.subset_entries(idx[:n_split])
