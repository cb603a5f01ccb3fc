"""The forward side of ``deeprank2_amd.ensemble``: ``FusedEnsembleForward``
(grids (max B_k, K) of forward-only rows of ``dr_ginet_multi_pass``, captured
into one HIP graph), ``predict_ensemble``, ``out_of_fold_predictions`` and the
validation of ``train_ensemble``.

Row k of each launch runs the code member k's own forward launch runs, on the
same arguments, so nothing here has a tolerance: every member's rows equal
(``torch.equal``) ``FusedFn.apply`` of that member alone, batch by batch.  The
graphs are the zoo of ``test_gpu_ensemble.py`` (the same records, built here).
"""

from __future__ import annotations

import contextlib
import copy
import functools

import numpy as np
import pytest
import torch

from deeprank2_amd import ensemble
from deeprank2_amd.engine import FusedTrainStep
from deeprank2_amd.ensemble import FusedEnsembleForward, ensemble_stats, epoch_batches, kfold_indices, out_of_fold_predictions, predict_ensemble, train_ensemble
from deeprank2_amd.fused import BatchHandle
from deeprank2_amd.neuralnets.gnn import ginet as amd
from deeprank2_amd.store import GraphRecord, GraphStore, pack_graphs
from deeprank2_amd.utils.synthetic import doubled_edges, make_dataset

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _syn(n_graphs, seed, f, **kw):
    out = []
    for i, g in enumerate(make_dataset(n_graphs, seed=seed, n_feat=f, **kw)):
        ei, ea = doubled_edges(g)
        out.append(GraphRecord(x=g["x"], edge_index=ei, edge_attr=ea, cluster0=g["cluster0"], cluster1=g["cluster1"], y=float(g["y"]), name=f"syn{seed}_{i}"))
    return out


def _hand(rng, n, f, edges, c0, c1, name):
    """A hand-made graph: ``edges`` are directed (i, j) columns of edge_index, stored once each, in this order."""
    ei = np.asarray(edges, np.int64).reshape(-1, 2).T
    ea = np.stack([rng.uniform(3.0, 9.0, size=ei.shape[1]), np.ones(ei.shape[1]), np.zeros(ei.shape[1])], axis=1).astype(np.float32)
    return GraphRecord(x=rng.normal(size=(n, f)).astype(np.float32), edge_index=np.ascontiguousarray(ei), edge_attr=ea, cluster0=np.asarray(c0, np.int64), cluster1=np.asarray(c1, np.int64), y=float(rng.uniform()), name=name)


@functools.lru_cache(maxsize=None)
def _zoo(f):
    """By position: 0 a 17-node residue graph; 1 one node; 2 twenty nodes and
    no edge; 3-6 N = 15, 16, 17, 33; 7 a row with a repeated neighbour; 8 a
    directed ring with chords (asymmetric: the transpose is not aliased);
    9, 10 two ~60-node residue graphs with two depth-1 clusters."""
    rng = np.random.default_rng(177 + f)
    ring = np.arange(24)
    recs = _syn(1, 900, f, n_lo=17, n_hi=17, mean_degree=6.0, k_lo=2, k_hi=3)
    recs.append(_hand(rng, 1, f, [], [0], [0], "one_node"))
    recs.append(_hand(rng, 20, f, [], np.arange(20) % 3, [0, 0, 0], "no_edges"))
    for n in (15, 16, 17, 33):
        recs += _syn(1, 500 + n, f, n_lo=n, n_hi=n, mean_degree=6.0, k_lo=2, k_hi=5)
    recs.append(_hand(rng, 10, f, [(0, 1), (0, 2), (0, 1), (3, 0), (0, 1), (5, 6), (6, 5), (9, 9)], np.arange(10) % 2, [0, 0], "repeated"))
    recs.append(_hand(rng, 24, f, np.concatenate([np.stack([ring, (ring + 1) % 24], 1), np.stack([ring, (ring + 5) % 24], 1)]), ring % 6, np.arange(6) % 3, "ring_chords"))
    for r in _syn(2, 901, f, n_lo=55, n_hi=65, mean_degree=10.0, k_lo=6, k_hi=8):
        r.cluster1 = np.arange(int(r.cluster0.max()) + 1, dtype=np.int64) % 2
        recs.append(r)
    return tuple(recs)


@functools.lru_cache(maxsize=None)
def _records24():
    recs = [*_zoo(30), *_syn(13, 902, 30, n_lo=12, n_hi=40, mean_degree=6.0, k_lo=2, k_hi=4)]
    assert len(recs) == 24  # noqa: PLR2004
    return tuple(recs)


@functools.lru_cache(maxsize=None)
def _store(f, out_dim, use_z):
    """One resident store per configuration (the forward only reads it)."""
    packed = pack_graphs(list(_zoo(f)))
    store = GraphStore(packed, DEV)
    if out_dim == 2:  # noqa: PLR2004
        store.set_targets(np.arange(packed.n_graphs) % 2)
    store.use_agg_x = use_z
    return store


@functools.lru_cache(maxsize=None)
def _store24():
    return GraphStore(pack_graphs(list(_records24())), DEV)


# member k's batches (graph ids of the zoo): sizes 7, 4, 1 and a short last
# batch; members with one, two and three batches; the one-node (1), edgeless
# (2) and asymmetric (8) graphs; graphs shared between members
_BATCHES = [
    [[9, 1, 4, 7, 10, 2, 8], [3, 5, 0, 6, 1, 2, 8], [6, 0]],
    [[1, 2, 9, 6], [8, 1, 2, 9], [5]],
    [[2], [1], [10]],
    [[10, 9, 8, 7, 6, 5, 4], [3, 2, 1, 0]],
    [[5, 3, 8, 1]],
    [[8, 8, 1, 2, 0, 4, 6], [8]],
    [[0, 4, 6, 10], [7, 2, 1, 3], [9, 5]],
    [[7, 2, 1, 3, 9, 5, 8], [2, 7, 0, 1, 10, 4, 6], [6, 10, 3]],
]
# other graph ids of the same sizes (the replay)
_BATCHES2 = [[[(g * 3 + 1 + m) % 11 for g in b] for b in bs] for m, bs in enumerate(_BATCHES)]


def _models(k, f, out_dim, train=True):
    """Members as a training run leaves them: train() mode, dropout 0.4."""
    models = []
    for i in range(k):
        torch.manual_seed(100 + i)
        m = amd.GINet(f, out_dim, 3).to(DEV).train(train)
        m._drop_seed = 7000 + 13 * i  # noqa: SLF001
        models.append(m)
    return models


def _alone(model, store, ids):
    """Member's own forward launch on one batch (no dropout)."""
    h = BatchHandle(store, np.asarray(ids, np.int32))
    with torch.no_grad():
        return amd.FusedFn.apply(amd.SPEC, h, None, model.output_shape, *model.ordered_params())


def _assert_rows(outs, models, store, batches, what=""):
    for m, (model, bs) in enumerate(zip(models, batches)):
        assert outs[m].shape == (sum(len(b) for b in bs), model.output_shape)
        o = 0
        for s, b in enumerate(bs):
            ref = _alone(model, store, b)
            assert torch.equal(outs[m][o : o + len(b)], ref), f"{what}member {m} batch {s}"
            assert bool(torch.isfinite(ref).all())
            o += len(b)


@pytest.mark.parametrize("use_z", [True, False], ids=["z", "gather"])
@pytest.mark.parametrize("out_dim", [1, 2])
@pytest.mark.parametrize("f", [30, 33])
@pytest.mark.parametrize("k", [1, 2, 3, 8])
def test_forward_rows_equal_each_members_own_forward(k, f, out_dim, use_z):
    models = _models(k, f, out_dim)
    store = _store(f, out_dim, use_z)
    batches = _BATCHES[:k]
    runner = FusedEnsembleForward(models, store, [[len(b) for b in bs] for bs in batches], fused=True)
    outs = runner.run(batches)
    assert runner.last_path == "fused" and runner.graph is not None
    assert (store._agg_x is not None) == use_z  # noqa: SLF001
    assert runner.out.shape == (k, max(sum(len(b) for b in bs) for bs in batches), out_dim)
    _assert_rows(outs, models, store, batches)
    if k > 1:  # the members did not all compute the same thing
        assert not torch.equal(_alone(models[0], store, [0, 4]), _alone(models[1], store, [0, 4]))
    # a second run on other graphs of the same sizes replays the captured graph
    g = runner.graph
    outs = runner.run(_BATCHES2[:k])
    assert runner.graph is g and runner.last_path == "fused"
    _assert_rows(outs, models, store, _BATCHES2[:k], "replay: ")


def test_eager_fused_and_sequential_runs_give_the_same_bits():
    k, f = 3, 30
    models = _models(k, f, 1)
    store = _store(f, 1, True)
    sizes = [[len(b) for b in bs] for bs in _BATCHES[:k]]
    got = {}
    for name, kw in {"captured": dict(fused=True), "eager": dict(fused=True, captured=False), "sequential": dict(fused=False)}.items():
        r = FusedEnsembleForward(models, store, sizes, **kw)
        got[name] = [o.clone() for o in r.run(_BATCHES[:k])]
        assert r.last_path == ("sequential" if name == "sequential" else "fused")
        assert (r.graph is not None) == (name == "captured")
    for name in ("eager", "sequential"):
        for a, b in zip(got["captured"], got[name]):
            assert torch.equal(a, b), name
    with pytest.raises(ValueError, match="do not match"):
        r.run([bs[:1] for bs in _BATCHES[:k]])
    with pytest.raises(ValueError, match="outside the store"):
        r.run([[[11] * len(b) for b in bs] for bs in _BATCHES[:k]])


def _state(models, steps):
    return [t.detach().clone() for m in models for t in m.state_dict().values()] + [t.detach().clone() for st in steps for t in st._state_tensors()]  # noqa: SLF001


def test_predicting_leaves_the_members_alone():
    """Members in train() mode with dropout 0.4, each with a FusedTrainStep that
    has stepped once: nothing of them changes, and the predictions are the
    eval-mode forward's (no dropout)."""
    k, f = 3, 30
    models = _models(k, f, 1)
    store = _store(f, 1, True)
    steps = [FusedTrainStep(m, lr=1e-3) for m in models]
    for st in steps:
        st.step(BatchHandle(store, np.asarray([0, 3, 4], np.int32)))
    torch.cuda.synchronize()
    before = _state(models, steps)
    counts = [(m._drop_calls, st.step_count) for m, st in zip(models, steps)]  # noqa: SLF001
    pred = predict_ensemble(models, store, batch_size=4)
    torch.cuda.synchronize()
    for n, (a, b) in enumerate(zip(_state(models, steps), before)):
        assert torch.equal(a, b), f"state tensor {n} changed"
    assert all(m.training and m.dropout == 0.4 for m in models)  # noqa: PLR2004
    assert counts == [(m._drop_calls, st.step_count) for m, st in zip(models, steps)]  # noqa: SLF001
    assert int(steps[0].counter[0]) == 1
    for m, model in enumerate(models):
        evalm = copy.deepcopy(model).eval()
        with torch.no_grad():
            ref = torch.cat([evalm(ensemble._Handle(BatchHandle(store, b.astype(np.int32)))) for b in epoch_batches(np.arange(11), 4, False, 0, 0, 0)])  # noqa: SLF001
        assert torch.equal(pred.members[m], ref), f"member {m}"


@contextlib.contextmanager
def _torch_ops_deterministic():
    """The layer path a non-finite GINet batch takes sums with torch's
    ``index_add`` (float atomics unless the deterministic algorithms are asked
    for): without this two runs of the same forward differ in the last bit."""
    before = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(True, warn_only=True)
    try:
        yield
    finally:
        torch.use_deterministic_algorithms(before[0], warn_only=before[1])


@pytest.mark.parametrize("why", ["force_large", "nonfinite"])
def test_ineligible_runs_fall_back_and_match(why):
    k, f = 3, 30
    models = _models(k, f, 1)
    batches = _BATCHES[:k]
    sizes = [[len(b) for b in bs] for bs in batches]
    if why == "nonfinite":
        recs = [copy.copy(r) for r in _zoo(f)]
        x = recs[4].x.copy()
        x[3, 2] = np.inf
        recs[4].x = x
        store = GraphStore(pack_graphs(recs), DEV)
    else:
        store = _store(f, 1, True)
    runner = FusedEnsembleForward(models, store, sizes, fused=True)
    if why == "force_large":
        runner.handles[1][0].force_large = True
    with _torch_ops_deterministic():
        outs = runner.run(batches)
        assert runner.last_path == "sequential" and runner.graph is None
        # the per-member result: model(batch) in eval mode, on a copy of the member
        for m, (model, bs) in enumerate(zip(models, batches)):
            evalm = copy.deepcopy(model).eval()
            o = 0
            for s, b in enumerate(bs):
                h = BatchHandle(store, np.asarray(b, np.int32))
                h.force_large = why == "force_large" and (m, s) == (1, 0)
                with torch.no_grad():
                    ref = evalm(ensemble._Handle(h))  # noqa: SLF001
                # (a non-finite batch may hold NaN: compared as bits)
                assert torch.equal(outs[m][o : o + len(b)].view(torch.int32), ref.view(torch.int32)), f"member {m} batch {s}"
                o += len(b)
    assert all(m.training for m in models)
    if why == "nonfinite":
        assert BatchHandle(store, np.asarray(batches[0][0], np.int32)).nonfinite
    else:
        runner.handles[1][0].force_large = False
        outs = runner.run(batches)
        assert runner.last_path == "fused"
        _assert_rows(outs, models, store, batches)


@pytest.mark.parametrize("out_dim", [1, 2])
def test_predict_ensemble(out_dim):
    k, f = 4, 30
    models = _models(k, f, out_dim)
    store = _store(f, out_dim, True)
    idx = np.asarray([10, 3, 8, 1, 2, 0, 7, 5, 9, 4], np.int64)  # 10 graphs in batches of 4: a short last batch
    pred = predict_ensemble(models, store, indices=idx, batch_size=4)
    assert pred.members.shape == (k, 10, out_dim) and np.array_equal(pred.indices, idx)
    batches = [b.tolist() for b in epoch_batches(idx, 4, False, 0, 0, 0)]
    _assert_rows(list(pred.members), models, store, [batches] * k)
    task = "classif" if out_dim == 2 else "regress"  # noqa: PLR2004
    mean, spread, label = ensemble_stats(pred.members, task)
    assert torch.equal(pred.mean, mean) and torch.equal(pred.spread, spread)
    if task == "classif":
        assert torch.equal(pred.label, label) and pred.spread.shape == (10,) and bool((pred.label >= 0).all())
    else:
        assert pred.label is None and label is None and pred.spread.shape == (10, 1)
        torch.testing.assert_close(pred.mean, pred.members.mean(0), rtol=1e-4, atol=1e-4)
    # the task can be chosen; the default covers every graph of the store, in order
    logits = predict_ensemble(models, store, batch_size=4, task="regress")
    assert logits.label is None and logits.mean.shape == (11, out_dim) and np.array_equal(logits.indices, np.arange(11))
    assert torch.equal(pred.members[:, 1], logits.members[:, 3]) and torch.equal(pred.members[:, 5], logits.members[:, 0])
    # predicting other graphs in batches of the same sizes runs the runner kept with
    # the store again (replays its graph when it has one); the first answer stays as it was
    runner = ensemble._runner_for(models, store, [[4, 4, 2]] * k)  # noqa: SLF001
    kept, graph = pred.members.clone(), runner.graph
    again = predict_ensemble(models, store, indices=idx[::-1].copy(), batch_size=4)
    assert ensemble._runner_for(models, store, [[4, 4, 2]] * k) is runner and runner.graph is graph  # noqa: SLF001
    assert torch.equal(pred.members, kept) and torch.equal(again.members, kept.flip(1)) and torch.equal(again.mean, pred.mean.flip(0))
    with pytest.raises(ValueError, match="task"):
        predict_ensemble(models, store, task="rank")


def test_back_to_back_predictions_without_a_sync():
    """``predict_ensemble`` returns without a device sync and its runner is
    kept with the store, so a loop over chunks of one size reuses one pinned
    id buffer while the stream is still behind the host.  Each call must be
    answered on its own ids: the stream is kept busy first, so that the host
    does run ahead, and nothing is read back until every call is queued."""
    k = 3
    store = _store(30, 1, True)
    models = _models(k, 30, 1)
    chunks = [np.asarray(c, np.int64) for c in ([0, 3, 4, 5, 6, 9], [10, 8, 7, 2, 1, 0], [5, 5, 9, 1, 3, 2], [6, 4, 10, 0, 8, 7])]
    refs = [[torch.cat([_alone(m, store, b) for b in epoch_batches(c, 4, False, 0, 0, 0)]) for m in models] for c in chunks]
    predict_ensemble(models, store, indices=chunks[-1], batch_size=4)  # the runner exists and its graph is captured
    busy = torch.randn(4096, 4096, device=DEV)
    torch.cuda.synchronize()
    for _ in range(20):  # tens of milliseconds of queued work ahead of the predictions
        busy = busy @ busy * 1e-3
    preds = [predict_ensemble(models, store, indices=c, batch_size=4) for c in chunks]
    torch.cuda.synchronize()
    for n, (p, ref) in enumerate(zip(preds, refs)):
        for m in range(k):
            assert torch.equal(p.members[m], ref[m]), f"call {n} member {m}"
        assert torch.equal(p.mean, ensemble_stats(torch.stack(ref), "regress")[0]), f"call {n}: mean"
    ensemble.forget_runners(store)
    assert "_dr_ens_forward" not in store.__dict__


def test_out_of_fold_predictions():
    k = 3
    store = _store24()
    models = _models(k, 30, 1)
    val_idx = [v for _, v in kfold_indices(23, k, seed=4)]
    pred, member = out_of_fold_predictions(models, store, val_idx, batch_size=5)
    assert pred.shape == (24, 1) and pred.dtype == torch.float32 and member.shape == (24,) and member.dtype == torch.int64
    for m, v in enumerate(val_idx):
        assert bool((member[torch.from_numpy(v).to(DEV)] == m).all())
        for b in epoch_batches(v, 5, False, 0, 0, 0):
            assert torch.equal(pred[torch.from_numpy(b).to(DEV)], _alone(models[m], store, b)), f"member {m}"
    assert int(member[23]) == -1 and bool(torch.isnan(pred[23]).all())
    assert int(torch.isnan(pred).sum()) == 1
    with pytest.raises(ValueError, match="held out more than once"):
        out_of_fold_predictions(models, store, [val_idx[0], val_idx[0], val_idx[2]])


def test_train_ensemble_validates_through_the_fused_runner():
    k, nepoch, bs = 3, 2, 5
    store = _store24()
    folds = kfold_indices(23, k, seed=4)
    train_idx, val_idx = [t for t, _ in folds], [v for _, v in folds]
    models = _models(k, 30, 1)
    alone = [copy.deepcopy(m) for m in models]
    res = train_ensemble(models, store, member_indices=train_idx, nepoch=nepoch, batch_size=bs, shuffle=True, seed=9, val_indices=val_idx, optimizer="adamw", loss="mse", val_fused=True)
    assert res.val_path == "fused" and res.val_loss.shape == (nepoch, k) and np.isfinite(res.val_loss).all()
    assert all(m.training for m in models)
    # the parent's loop on the same members after the final epoch
    for m, model in enumerate(models):
        st = FusedTrainStep(model, optimizer="adamw", loss="mse", max_batch=bs)
        assert ensemble._held_out_loss(st, store, val_idx[m], bs) == res.val_loss[nepoch - 1, m], f"member {m}"  # noqa: SLF001
    # fused = False: the members' own loops, the same numbers
    seq = train_ensemble(alone, store, member_indices=train_idx, nepoch=nepoch, batch_size=bs, shuffle=True, seed=9, val_indices=val_idx, optimizer="adamw", loss="mse", fused=False)
    assert seq.val_path == "sequential" and np.array_equal(seq.val_loss, res.val_loss) and np.array_equal(seq.train_loss, res.train_loss)
    assert train_ensemble(_models(2, 30, 1), store, nepoch=1, batch_size=8).val_path is None
