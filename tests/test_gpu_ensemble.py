"""Several GINet members stepped by one pair of launches
(``deeprank2_amd.ensemble``: ``dr_ginet_multi_pass`` + ``dr_reduce_update_multi``).

Row k of each launch runs the code member k's own launch runs, on the same
arguments in the same order, so nothing here has a tolerance: every member's
parameters, optimizer state, two-word step counter, loss and outputs equal
(``torch.equal``) those of a ``FusedTrainStep`` of its own fed the same batches.
"""

from __future__ import annotations

import contextlib
import copy
import functools

import numpy as np
import pytest
import torch

from deeprank2_amd.engine import FusedTrainStep
from deeprank2_amd.ensemble import FusedEnsembleStep, epoch_batches, kfold_indices, train_ensemble
from deeprank2_amd.fused import BatchHandle
from deeprank2_amd.neuralnets.gnn import ginet as amd
from deeprank2_amd.neuralnets.gnn.foutnet import FoutNet
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
def _zoo_packed(f):
    return pack_graphs(list(_zoo(f)))


# member k's batch at each of the three steps: sizes 7, 4, 1, ...; the one-node
# and the edgeless graph; members 0 and 1 (and 3) share graphs; every graph of
# the zoo; a batch that changes size between steps (another reduce argument buffer)
_BATCHES = [
    [[9, 1, 4, 7, 10, 2, 8], [9, 1, 4, 7, 10, 2, 8], [3, 5, 0]],
    [[1, 2, 9, 6], [6, 1, 2, 9], [1, 2, 9, 6]],
    [[2], [1], [10]],
    [[10, 9, 8, 7, 6, 5, 4, 3, 2, 1, 0]] * 3,
    [[5, 3], [0, 6], [5, 3]],
    [[8, 8, 1], [8, 8, 1], [8, 8, 1]],
    [[0, 4, 6, 10, 7], [0, 4, 6, 10, 7], [0, 4, 6, 10, 7]],
    [[7, 2, 1, 3, 9, 5], [2, 7], [7, 2, 1, 3, 9, 5]],
]

_LOSSES = {"mse": dict(loss="mse"), "huber": dict(loss="huber", loss_param=0.3), "ce": dict(loss="ce", class_weights=[0.3, 0.7])}


def _models(k, f, out_dim):
    models = []
    for i in range(k):
        torch.manual_seed(100 + i)
        m = amd.GINet(f, out_dim, 3).to(DEV).train()
        m._drop_seed = 7000 + 13 * i  # noqa: SLF001
        models.append(m)
    return models


def _hyper(k):
    return [1e-3 * (1 + i) for i in range(k)], [1e-5 * (3 * i) for i in range(k)]  # (member 0: no weight decay)


def _store(f, out_dim, use_z=True):
    packed = _zoo_packed(f)
    store = GraphStore(packed, DEV)
    if out_dim == 2:  # noqa: PLR2004
        store.set_targets(np.arange(packed.n_graphs) % 2)
    store.use_agg_x = use_z
    return store


@functools.lru_cache(maxsize=None)
def _shared_store(f, out_dim, use_z):
    """One resident store per configuration for the cases that only read it."""
    return _store(f, out_dim, use_z)


def _handles(store, step_no, k):
    return [BatchHandle(store, np.asarray(_BATCHES[i][step_no], np.int32)) for i in range(k)]


def _assert_member_equals(st: FusedTrainStep, ref: FusedTrainStep, what):
    for n, (a, b) in enumerate(zip(st.params, ref.params)):
        assert torch.equal(a, b), f"{what}: parameter {n}"
    for n, ((m1, v1), (m2, v2)) in enumerate(zip(st.states, ref.states)):
        assert torch.equal(m1, m2), f"{what}: exp_avg {n}"
        assert torch.equal(v1, v2), f"{what}: exp_avg_sq / exp_inf {n}"
    assert torch.equal(st.counter, ref.counter), f"{what}: step counter"


@pytest.mark.parametrize("use_z", [True, False], ids=["z", "gather"])
@pytest.mark.parametrize("loss", sorted(_LOSSES))
@pytest.mark.parametrize("optimizer", ["adam", "adamw", "adamax"])
@pytest.mark.parametrize("f", [30, 33])
@pytest.mark.parametrize("k", [1, 2, 3, 8])
def test_ensemble_step_equals_separate_steps(k, f, optimizer, loss, use_z):
    out_dim = 2 if loss == "ce" else 1
    models = _models(k, f, out_dim)
    alone = [copy.deepcopy(m) for m in models]
    lrs, wds = _hyper(k)
    ens = FusedEnsembleStep(models, lr=lrs, weight_decay=wds, optimizer=optimizer, max_batch=4, **_LOSSES[loss])
    refs = [FusedTrainStep(m, lr=lrs[i], weight_decay=wds[i], optimizer=optimizer, max_batch=4, **_LOSSES[loss]) for i, m in enumerate(alone)]
    store = _shared_store(f, out_dim, use_z)
    for s in range(3):
        hs = _handles(store, s, k)
        losses, outs = ens.step(hs)
        assert ens.last_path == "fused"
        assert (store._agg_x is not None) == use_z  # noqa: SLF001
        for i, ref in enumerate(refs):
            rl, ro = ref.step(hs[i])
            assert torch.equal(losses[i : i + 1], rl), f"step {s} member {i}: loss"
            assert torch.equal(outs[i], ro), f"step {s} member {i}: out"
            _assert_member_equals(ens.steps[i], ref, f"step {s} member {i}")
            assert bool(torch.isfinite(rl).all()) and ens.steps[i].step_count == s + 1
    assert int(refs[0].counter[0]) == 3  # noqa: PLR2004
    # the members did not all compute the same thing
    if k > 1:
        assert not torch.equal(ens.steps[0].params[12], ens.steps[1].params[12])


def test_member_sitting_out_is_untouched():
    k, f = 3, 30
    models = _models(k, f, 1)
    alone = [copy.deepcopy(m) for m in models]
    lrs, wds = _hyper(k)
    ens = FusedEnsembleStep(models, lr=lrs, weight_decay=wds)
    refs = [FusedTrainStep(m, lr=lrs[i], weight_decay=wds[i]) for i, m in enumerate(alone)]
    store = _store(f, 1)
    for s in range(3):
        hs = _handles(store, s, k)
        if s == 1:
            hs[1] = None
            before = [t.detach().clone() for t in ens.steps[1]._state_tensors()]  # noqa: SLF001
            loss_before = ens.losses[1].clone()
        _, outs = ens.step(hs)
        assert ens.last_path == "fused"
        if s == 1:
            assert outs[1] is None
            for n, (a, b) in enumerate(zip(ens.steps[1]._state_tensors(), before)):  # noqa: SLF001
                assert torch.equal(a, b), f"state tensor {n} of the absent member changed"
            assert torch.equal(ens.losses[1], loss_before) and ens.steps[1].step_count == 1
        for i, ref in enumerate(refs):
            if hs[i] is not None:
                ref.step(hs[i])
    torch.cuda.synchronize()
    for i, ref in enumerate(refs):
        _assert_member_equals(ens.steps[i], ref, f"member {i}")
    assert int(ens.steps[1].counter[0]) == 2 and int(ens.steps[0].counter[0]) == 3  # noqa: PLR2004
    # every member absent: nothing runs
    snap = [t.detach().clone() for st in ens.steps for t in st._state_tensors()]  # noqa: SLF001
    ens.step([None] * k)
    for a, b in zip([t for st in ens.steps for t in st._state_tensors()], snap):  # noqa: SLF001
        assert torch.equal(a, b)


def test_captured_ensemble_step_replays_like_eager():
    k, f = 4, 30
    lrs, wds = _hyper(k)
    one = FusedEnsembleStep(_models(k, f, 1), lr=lrs, weight_decay=wds)
    two = FusedEnsembleStep(_models(k, f, 1), lr=lrs, weight_decay=wds)
    store = _store(f, 1)
    hs = _handles(store, 0, k)
    hs[2] = None  # (a captured step with an empty row)
    assert store._agg_x is None  # noqa: SLF001
    g = one.capture(hs)
    assert one.last_path == "fused" and store._agg_x is not None  # noqa: SLF001
    for st in one.steps:  # capturing left the training state alone
        assert int(st.counter[0]) == 0 and st.step_count == 0
    for _ in range(3):
        g.replay()
        two.step(hs)
    torch.cuda.synchronize()
    for i in range(k):
        _assert_member_equals(one.steps[i], two.steps[i], f"member {i}")
        if hs[i] is not None:
            assert torch.equal(one.steps[i].out[: hs[i].B], two.steps[i].out[: hs[i].B])
    assert torch.equal(one.losses, two.losses)
    assert [int(st.counter[0]) for st in one.steps] == [3, 3, 0, 3]


@contextlib.contextmanager
def _torch_ops_deterministic(on):
    """The layer path a non-finite GINet batch takes sums with torch's
    ``index_add``, float atomics unless torch's deterministic algorithms are
    asked for: two runs of the SAME member step otherwise differ in the last
    bit, and no comparison of two runs could ask for equality."""
    before = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    if on:
        torch.use_deterministic_algorithms(True, warn_only=True)
    try:
        yield
    finally:
        torch.use_deterministic_algorithms(before[0], warn_only=before[1])


@pytest.mark.parametrize("why", ["force_large", "nonfinite"])
def test_ineligible_batches_fall_back_and_match(why):
    k, f = 3, 30
    if why == "nonfinite":
        recs = [copy.copy(r) for r in _zoo(f)]
        x = recs[4].x.copy()
        x[3, 2] = np.inf
        recs[4].x = x
        store = GraphStore(pack_graphs(recs), DEV)
    else:
        store = _store(f, 1)
    models = _models(k, f, 1)
    alone = [copy.deepcopy(m) for m in models]
    ens = FusedEnsembleStep(models)
    refs = [FusedTrainStep(m) for m in alone]
    with _torch_ops_deterministic(why == "nonfinite"):
        for s in range(2):
            hs = _handles(store, s, k)  # (member 0's batches hold graph 4)
            ref_hs = _handles(store, s, k)
            if why == "force_large":
                hs[1].force_large = ref_hs[1].force_large = True
            else:
                assert hs[0].nonfinite and not hs[1].nonfinite
            # (the layer path a non-finite batch takes draws its dropout from torch's
            # generator, not from the member's counter hash: the same draws on both sides)
            torch.manual_seed(50 + s)
            losses, outs = ens.step(hs)
            assert ens.last_path == "sequential"
            torch.manual_seed(50 + s)
            for i, ref in enumerate(refs):
                rl, ro = ref.step(ref_hs[i])
                # (a non-finite batch may leave NaN / inf behind: compared as bits)
                assert torch.equal(losses[i : i + 1].view(torch.int32), rl.view(torch.int32)), f"member {i}: loss"
                assert torch.equal(outs[i].view(torch.int32), ro.view(torch.int32)), f"member {i}: out"
                for n, (a, b) in enumerate(zip(ens.steps[i].params, ref.params)):
                    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"member {i}: parameter {n}"
                assert torch.equal(ens.steps[i].counter, ref.counter)
    # the eligible batches of the same ensemble then take the fused launches again
    clean = _store(f, 1)
    ens.step(_handles(clean, 2, k))
    assert ens.last_path == "fused"


def test_train_ensemble_matches_sequential_loops():
    f, k, nepoch, bs = 30, 3, 2, 5
    recs = [*_zoo(f), *_syn(13, 902, f, n_lo=12, n_hi=40, mean_degree=6.0, k_lo=2, k_hi=4)]
    assert len(recs) == 24  # noqa: PLR2004
    store = GraphStore(pack_graphs(recs), DEV)
    folds = kfold_indices(23, k, seed=4)  # 23 of the 24: folds of 8, 8, 7 -> training parts of 15, 15, 16 graphs (3, 3 and 4 batches)
    train_idx, val_idx = [t for t, _ in folds], [v for _, v in folds]
    assert sorted(len(t) for t in train_idx) == [15, 15, 16]
    models = _models(k, f, 1)
    alone = [copy.deepcopy(m) for m in models]
    lrs, wds = _hyper(k)
    res = train_ensemble(models, store, member_indices=train_idx, nepoch=nepoch, batch_size=bs, shuffle=True, seed=9, val_indices=val_idx, lr=lrs, weight_decay=wds, optimizer="adamw", loss="mse")
    assert res.train_loss.shape == (nepoch, k) and res.val_loss.shape == (nepoch, k) and res.models is not None
    assert np.isfinite(res.train_loss).all() and np.isfinite(res.val_loss).all()
    for i, m in enumerate(alone):
        ref = FusedTrainStep(m, lr=lrs[i], weight_decay=wds[i], optimizer="adamw", loss="mse", max_batch=bs)
        for e in range(nepoch):
            total, count = torch.zeros((), dtype=torch.float64, device=DEV), 0
            for idx in epoch_batches(train_idx[i], bs, True, 9, i, e):
                loss, _ = ref.step(BatchHandle(store, idx.astype(np.int32)))
                total += loss[0].double() * len(idx)
                count += len(idx)
            assert float(total.item()) / count == res.train_loss[e, i], f"member {i} epoch {e}"
        for n, (a, b) in enumerate(zip(models[i].ordered_params(), ref.params)):
            assert torch.equal(a, b), f"member {i}: parameter {n}"
        # the held-out loss: the member's forward-only pass in eval mode, MSE by torch
        m.eval()
        h = BatchHandle(store, val_idx[i].astype(np.int32))
        with torch.no_grad():
            total = 0.0
            for idx in epoch_batches(val_idx[i], bs, False, 0, 0, 0):
                hb = BatchHandle(store, idx.astype(np.int32))
                out = amd.FusedFn.apply(amd.SPEC, hb, None, 1, *ref.params)
                y = torch.from_numpy(np.asarray(store.packed.y)[idx]).to(DEV, torch.float32)
                total += float(torch.nn.functional.mse_loss(out.reshape(-1), y).double()) * len(idx)
        assert h.B in (7, 8)
        assert res.val_loss[nepoch - 1, i] == total / h.B


def test_constructor_refusals():
    g = lambda f=30, out=1: amd.GINet(f, out, 3).to(DEV)  # noqa: E731
    with pytest.raises(ValueError, match="input_shape"):
        FusedEnsembleStep([g(30), g(33)])
    with pytest.raises(ValueError, match="GINet"):
        FusedEnsembleStep([g(), FoutNet(30, 1).to(DEV)])
    with pytest.raises(ValueError, match="1 to 8 members"):
        FusedEnsembleStep([g() for _ in range(9)])
    with pytest.raises(ValueError, match="fp32"):
        FusedEnsembleStep([g(), g()], compute_dtype="bf16")
    a, b = BatchHandle(_store(30, 1), np.asarray([0, 1], np.int32)), BatchHandle(_store(30, 1), np.asarray([0, 1], np.int32))
    with pytest.raises(ValueError, match="one GraphStore"):
        FusedEnsembleStep([g(), g()]).step([a, b])
