"""Validation formed on the device: ``FusedEnsembleForward(score=...)`` (one
``dr_ensemble_score`` as the run's last launch), ``train_ensemble`` with
``val_loss="device"``, ``patience`` and ``restore_best``, and
``score_ensemble``.

The graphs are the zoo of ``test_gpu_ensemble_forward.py`` (the same records,
built here: 1 to 65 nodes, most between 15 and 65).  The MSE sums equal the
numpy restatement ``tests/score_ref.py`` bit for bit; the cross entropy is held
to the tolerance of ``test_gpu_ensemble_score.py`` (rtol 1e-5 plus 1e-6 *
max(1, max|logit|) per row).
"""

from __future__ import annotations

import copy
import functools

import numpy as np
import pytest
import torch
from score_ref import score_ref

from deeprank2_amd.ensemble import FusedEnsembleForward, MemberStopping, ScoreSpec, ensemble_score, epoch_batches, kfold_indices, predict_ensemble, score_ensemble, scores_from_sums, train_ensemble
from deeprank2_amd.neuralnets.gnn import ginet as amd
from deeprank2_amd.store import GraphRecord, GraphStore, pack_graphs
from deeprank2_amd.utils.synthetic import doubled_edges, make_dataset

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = 30


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
def _records24():
    """The 11 graphs of the forward tests' zoo (a 17-node residue graph; one
    node; twenty nodes and no edge; N = 15, 16, 17, 33; a repeated neighbour; a
    directed ring with chords; two ~60-node graphs) and 13 more of 12-40 nodes."""
    f = F
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
    recs += _syn(13, 902, f, n_lo=12, n_hi=40, mean_degree=6.0, k_lo=2, k_hi=4)
    assert len(recs) == 24  # noqa: PLR2004
    return tuple(recs)


@functools.lru_cache(maxsize=None)
def _store(out_dim):
    """One resident store per task (read only): regression targets, or the classes 0, 1, 1, 0, 1, 1 ..."""
    store = GraphStore(pack_graphs(list(_records24())), DEV)
    if out_dim == 2:  # noqa: PLR2004
        store.set_targets((np.arange(store.n_graphs) % 3 > 0).astype(np.float32))
    return store


def _models(k, out_dim):
    """Members as a training run leaves them: train() mode, dropout 0.4."""
    models = []
    for i in range(k):
        torch.manual_seed(100 + i)
        m = amd.GINet(F, out_dim, 3).to(DEV).train()
        m._drop_seed = 7000 + 13 * i  # noqa: SLF001
        models.append(m)
    return models


_BATCHES = [[[9, 1, 4, 7, 10, 2, 8], [3, 5, 0, 6, 1, 2, 8], [6, 0]], [[1, 2, 9, 6], [8, 1, 2, 9], [5]], [[2], [1], [10]]]
_BATCHES2 = [[[(g * 3 + 1 + m) % 24 for g in b] for b in bs] for m, bs in enumerate(_BATCHES)]
CW = [0.3, 1.7]


def _by_hand(views, store, batches, spec):
    """``ensemble_score`` called member by member on the runner's views."""
    rows, confs = [], []
    for v, bs in zip(views, batches):
        ids = torch.tensor([g for b in bs for g in b], dtype=torch.int64, device=DEV)
        s, c = ensemble_score(v, store.y, gids=ids, loss=spec.loss, loss_param=spec.loss_param, class_weights=spec.class_weights, confusion=spec.confusion)
        rows.append(s)
        confs.append(c)
    return torch.cat(rows), None if confs[0] is None else torch.cat(confs)


@pytest.mark.parametrize("out_dim", [1, 2])
def test_a_runner_with_a_score_ends_its_run_with_the_score_launch(out_dim):
    k = 3
    models, store = _models(k, out_dim), _store(out_dim)
    spec = ScoreSpec("mse") if out_dim == 1 else ScoreSpec("ce", class_weights=CW, confusion=True)
    sizes = [[len(b) for b in bs] for bs in _BATCHES]
    got = {}
    for name, kw in {"captured": dict(fused=True), "eager": dict(fused=True, captured=False), "sequential": dict(fused=False)}.items():
        r = FusedEnsembleForward(models, store, sizes, score=spec, **kw)
        views = r.run(_BATCHES)
        assert r.last_path == ("sequential" if name == "sequential" else "fused") and (r.graph is not None) == (name == "captured")
        got[name] = (r.sums.clone(), None if r.confusion is None else r.confusion.clone(), r.out.clone())
        hand_s, hand_c = _by_hand(views, store, _BATCHES, spec)
        assert torch.equal(r.sums, hand_s), name
        assert (r.confusion is None and out_dim == 1) or torch.equal(r.confusion, hand_c), name
        if name == "captured":  # other ids of the same sizes: the graph is replayed and gives that run's sums
            graph = r.graph
            views = r.run(_BATCHES2)
            assert r.graph is graph
            hand2, _ = _by_hand(views, store, _BATCHES2, spec)
            assert torch.equal(r.sums, hand2) and not torch.equal(hand2, hand_s)
    for name in ("eager", "sequential"):
        assert torch.equal(got["captured"][0], got[name][0]), name
        assert got[name][1] is None or torch.equal(got["captured"][1], got[name][1]), name
    assert bool(torch.isfinite(got["captured"][0]).all()) and got["captured"][0][:, 3].tolist() == [0.0] * k
    # the restatement on the same predictions
    ids = np.zeros((k, r.out.shape[1]), dtype=np.int64)
    for m, bs in enumerate(_BATCHES):
        ids[m, : r.n[m]] = [g for b in bs for g in b]
    want, wconf = score_ref(got["captured"][2].cpu().numpy(), store.y.cpu().numpy(), r.n, gids=ids, loss=spec.loss, class_w=None if out_dim == 1 else np.asarray(CW, np.float32))
    sums = got["captured"][0].cpu().numpy()
    if out_dim == 1:
        assert np.array_equal(sums, want)
    else:
        assert np.array_equal(sums[:, 1:], want[:, 1:]) and np.array_equal(got["captured"][1].cpu().numpy(), wconf)
        logit = float(got["captured"][2].abs().max())
        assert (np.abs(sums[:, 0] - want[:, 0]) <= 1e-5 * np.abs(want[:, 0]) + 1e-6 * max(1.0, logit) * np.asarray(r.n)).all()
    # without a score: no buffer, no launch, the same predictions
    plain = FusedEnsembleForward(models, store, sizes)
    plain.run(_BATCHES)
    assert not hasattr(plain, "sums") and plain.score is None and torch.equal(plain.out, got["captured"][2])


def _folds(k):
    folds = kfold_indices(24, k, seed=4)
    return [t for t, _ in folds], [v for _, v in folds]


def _params(models):
    return [p.detach().clone() for m in models for p in m.ordered_params()]


def _val_reference(models, store, val_idx, loss, class_w=None):
    """score_ref on the members' predictions of their held-out graphs."""
    batches = [epoch_batches(v, 5, False, 0, 0, 0) for v in val_idx]
    r = FusedEnsembleForward(models, store, [[len(b) for b in bs] for bs in batches])
    r.run(batches)
    ids = np.zeros((len(models), r.out.shape[1]), dtype=np.int64)
    for m, v in enumerate(val_idx):
        ids[m, : len(v)] = v
    sums, _ = score_ref(r.out.cpu().numpy(), store.y.cpu().numpy(), r.n, gids=ids, loss=loss, class_w=class_w)
    return sums, float(r.out.abs().max())


def test_train_ensemble_with_the_device_loss():
    k, nepoch, bs = 3, 2, 5
    store = _store(1)
    train_idx, val_idx = _folds(k)
    kw = dict(member_indices=train_idx, nepoch=nepoch, batch_size=bs, shuffle=True, seed=9, val_indices=val_idx, optimizer="adamw", loss="mse")
    base = _models(k, 1)
    runs = {}
    for name, extra in {"plain": {}, "host": dict(val_loss="host"), "device": dict(val_loss="device")}.items():
        models = [copy.deepcopy(m) for m in base]
        runs[name] = (train_ensemble(models, store, **kw, **extra), models)
    plain, host, dev = (runs[n][0] for n in ("plain", "host", "device"))
    # "host" is the call without the new arguments, bit for bit
    assert np.array_equal(host.val_loss, plain.val_loss) and np.array_equal(host.train_loss, plain.train_loss) and host.val_scores is None
    # the device loss changes nothing of the training
    assert np.array_equal(dev.train_loss, host.train_loss) and dev.val_path == "fused"
    for a, b in zip(_params(runs["device"][1]), _params(runs["host"][1])):
        assert torch.equal(a, b)
    # its values: the restatement on the final members' predictions, bit for bit (MSE)
    sums, _ = _val_reference(runs["device"][1], store, val_idx, "mse")
    assert len(dev.val_scores) == nepoch and np.array_equal(dev.val_loss[-1], sums[:, 0] / sums[:, 1])
    assert np.array_equal(dev.val_scores[-1].loss, dev.val_loss[-1]) and dev.val_scores[-1].n.tolist() == [len(v) for v in val_idx]
    assert np.array_equal(dev.val_scores[-1].rmse, np.sqrt(sums[:, 4] / sums[:, 1]))
    # and close to the host's sum of batch means (fp32 means of at most 5 terms, summed in double)
    np.testing.assert_allclose(dev.val_loss, host.val_loss, rtol=1e-6)
    assert dev.best_epoch.shape == (k,) and (dev.stopped_epoch == -1).all()


def test_the_device_loss_does_not_depend_on_the_batch_size():
    """The same members (lr = 0: the parameters never move) and held-out sets,
    cut into batches of 4 and of 7: the device's MSE values are equal."""
    k = 2
    store = _store(1)
    train_idx, val_idx = _folds(k)
    base = _models(k, 1)
    res = {}
    for bs in (4, 7):
        models = [copy.deepcopy(m) for m in base]
        res[bs] = train_ensemble(models, store, member_indices=train_idx, nepoch=1, batch_size=bs, val_indices=val_idx, lr=0.0, loss="mse", val_loss="device")
        for a, b in zip(_params(models), _params(base)):
            assert torch.equal(a, b)
    assert np.isfinite(res[4].val_loss).all() and (res[4].val_loss == res[7].val_loss).all()


def test_weighted_cross_entropy_is_the_loss_over_the_whole_held_out_set():
    k, bs = 2, 5
    store = _store(2)
    train_idx, val_idx = _folds(k)
    models = _models(k, 2)
    res = train_ensemble(models, store, member_indices=train_idx, nepoch=2, batch_size=bs, seed=3, val_indices=val_idx, loss="ce", class_weights=CW, val_loss="device")
    sums, logit = _val_reference(models, store, val_idx, "ce", np.asarray(CW, np.float32))
    want = sums[:, 0] / sums[:, 1]  # sum w_y l / sum w_y over the whole set, in float64
    n = np.asarray([len(v) for v in val_idx])
    tol = (1e-5 * np.abs(sums[:, 0]) + 1e-6 * max(1.0, logit) * n) / sums[:, 1]
    print("weighted ce: device", res.val_loss[-1], "reference", want, "tolerance", tol)
    assert (np.abs(res.val_loss[-1] - want) <= tol).all()
    y = store.y.cpu().numpy()
    assert np.array_equal(sums[:, 1], [np.asarray(CW, np.float32).astype(np.float64)[y[v].astype(int)].sum() for v in val_idx])
    assert np.isfinite(res.val_scores[-1].accuracy).all()


def _member_state(res, m):
    return [p.detach().clone() for p in res.models[m].ordered_params()] + [t.detach().clone() for t in res.step.steps[m]._state_tensors()]  # noqa: SLF001


def test_early_stopping_and_restore_best():
    """Member 1 has lr = 0: its validation loss never falls, so with patience 1
    it is stopped after epoch 1 and sits every later step out."""
    k, nepoch = 3, 3
    store = _store(1)
    train_idx, val_idx = _folds(k)
    kw = dict(member_indices=train_idx, batch_size=5, shuffle=True, seed=9, val_indices=val_idx, lr=[1e-3, 0.0, 1e-3], loss="mse")
    base = _models(k, 1)

    def run(n, **extra):
        return train_ensemble([copy.deepcopy(m) for m in base], store, nepoch=n, **kw, **extra)

    full = {n: run(n) for n in range(1, nepoch + 1)}  # no patience: the members after 1, 2 and 3 epochs
    for val_loss in ("host", "device"):
        res = run(nepoch, patience=1, min_delta=0.0, val_loss=val_loss)
        # the bookkeeping on the losses the run reports
        want = MemberStopping(k, 1, 0.0)
        for e in range(nepoch):
            want.update(e, res.val_loss[e])
        assert res.stopped_epoch.tolist() == want.stopped_epoch.tolist() and res.best_epoch.tolist() == want.best_epoch.tolist()
        assert res.stopped_epoch[1] == 1 and res.best_epoch[1] == 0
        assert np.isnan(res.val_loss[2, 1]) and np.isnan(res.train_loss[2, 1]) and np.isfinite(res.val_loss[:2, 1]).all()
        # every member is where a run of as many epochs as it trained leaves it: parameters, moments, counters
        for m in range(k):
            trained = nepoch if res.stopped_epoch[m] < 0 else int(res.stopped_epoch[m]) + 1
            for a, b in zip(_member_state(res, m), _member_state(full[trained], m)):
                assert torch.equal(a, b), (val_loss, m)
            if val_loss == "host":
                assert np.array_equal(res.val_loss[:trained, m], full[nepoch].val_loss[:trained, m])
    # restore_best: each member ends with the parameters it had after its best epoch
    res = run(nepoch, restore_best=True)
    assert (res.stopped_epoch == -1).all() and np.array_equal(res.val_loss, full[nepoch].val_loss)
    for m in range(k):
        for a, b in zip(res.models[m].ordered_params(), full[int(res.best_epoch[m]) + 1].models[m].ordered_params()):
            assert torch.equal(a, b), m
    with pytest.raises(ValueError, match="val_indices"):
        train_ensemble(_models(2, 1), store, nepoch=1, patience=1)


@pytest.mark.parametrize("k,out_dim", [(2, 1), (1, 1), (3, 2)])
def test_score_ensemble(k, out_dim):
    store = _store(out_dim)
    models = _models(k, out_dim)
    idx = np.array([3, 0, 9, 10, 4, 22, 17, 1, 2, 8, 15])
    loss = "mse" if out_dim == 1 else "ce"
    cw = None if out_dim == 1 else CW
    members, ens, pred = score_ensemble(models, store, idx, batch_size=4, loss=loss, class_weights=cw)
    ref = predict_ensemble(models, store, idx, batch_size=4)
    assert torch.equal(pred.members, ref.members) and torch.equal(pred.mean, ref.mean)
    gids = torch.from_numpy(idx).to(DEV)
    task = "regress" if out_dim == 1 else "classif"
    s, c = ensemble_score(ref.members, store.y, gids=gids, loss=loss, class_weights=cw, confusion=out_dim > 1)
    want = scores_from_sums(s.cpu().numpy(), None if c is None else c.cpu().numpy(), task)
    s, c = ensemble_score(ref.mean, store.y, gids=gids, loss=loss, class_weights=cw, confusion=out_dim > 1, probs=out_dim > 1)
    want_e = scores_from_sums(s.cpu().numpy(), None if c is None else c.cpu().numpy(), task)
    fields = ("loss", "n", "n_nan", "n_skipped") + (("rmse", "mae", "pearson", "r2") if out_dim == 1 else ("accuracy", "confusion", "mcc", "tpr", "tnr", "precision"))
    for f in fields:
        assert np.array_equal(getattr(members, f), getattr(want, f), equal_nan=True), f
        assert np.array_equal(getattr(ens, f), getattr(want_e, f), equal_nan=True), f
    assert members.loss.shape == (k,) and ens.loss.shape == (1,) and np.isfinite(members.loss).all() and np.isfinite(ens.loss).all()
    assert members.n.tolist() == [idx.size] * k and ens.n.tolist() == [idx.size]
    if k == 1:  # one member is its own ensemble
        for f in ("loss", "rmse", "mae", "pearson", "r2"):
            assert getattr(ens, f)[0] == getattr(members, f)[0], f
    if out_dim > 1:
        assert ens.confusion.shape == (1, 2, 2) and ens.confusion.sum() == idx.size
        with pytest.raises(ValueError, match="does not go with"):
            score_ensemble(models, store, idx, loss="mse", task="classif")
