"""What the captured runners share (``epoch.StagedBatches``,
``fused.capture_after_warmup``, ``FusedTrainStep._capture_steps``), directly:
two runs that follow one another without a device sync each see their own
graph ids, and an ``EpochRunner``'s first use leaves the training state where
eager steps leave it.  Nothing here has a tolerance: the runners make the
launches of the per-batch loop, on the same arguments.
"""

from __future__ import annotations

import copy
import functools

import numpy as np
import pytest
import torch

from deeprank2_amd.engine import FusedTrainStep
from deeprank2_amd.ensemble import _Handle
from deeprank2_amd.epoch import EpochRunner, EvalRunner, StagedBatches, eligible, eval_eligible
from deeprank2_amd.fused import BatchHandle
from deeprank2_amd.neuralnets.gnn.foutnet import FoutNet
from deeprank2_amd.neuralnets.gnn.ginet import GINet
from deeprank2_amd.store import GraphRecord, GraphStore, pack_graphs
from deeprank2_amd.utils.synthetic import doubled_edges, make_dataset

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = [4, 4, 3]
# two epochs' worth of graph ids in batches of SIZES: every graph once, then another order
B1 = [[9, 1, 4, 7], [10, 2, 8, 3], [5, 0, 6]]
B2 = [[(3 * g + 1) % 11 for g in b] for b in B1]


@functools.lru_cache(maxsize=None)
def _store():
    recs = []
    for i, g in enumerate(make_dataset(11, seed=903, n_feat=30, n_lo=25, n_hi=60, mean_degree=6.0, k_lo=2, k_hi=4)):
        ei, ea = doubled_edges(g)
        recs.append(GraphRecord(x=g["x"], edge_index=ei, edge_attr=ea, cluster0=g["cluster0"], cluster1=g["cluster1"], y=float(g["y"]), name=f"syn{i}"))
    return GraphStore(pack_graphs(recs), DEV)


def test_staged_batches_back_to_back_loads_each_gather_their_own_ids():
    store = _store()
    sizes = [SIZES, [2], []]
    st = StagedBatches(store, sizes)
    assert st.descs.shape == (3, 11, 64) and st.gids.shape == st.pin.shape == (3, 11)
    assert [len(hs) for hs in st.handles] == [3, 1, 0] and st.probe.B == 1
    loads = [[B1, [[6, 2]], []], [B2, [[0, 10]], []]]
    seen = []
    for batches in loads:  # no synchronize in between
        st.load([[np.asarray(b) for b in bs] for bs in batches])
        seen.append(st.descs.clone())
    torch.cuda.synchronize()
    for batches, descs in zip(loads, seen):
        for r, bs in enumerate(batches):
            for s, ids in enumerate(bs):
                o, h = int(st.offs[r][s]), st.handles[r][s]
                assert h.B == len(ids) and h.descs.data_ptr() == st.descs[r, o].data_ptr()
                assert torch.equal(descs[r, o : o + h.B].reshape(-1), store.descriptors(ids)), (r, s)
    # ids past a row's last graph, and the row without a batch, are never written
    assert not st.pin[1, 2:].any() and not st.pin[2].any()


@pytest.mark.parametrize("model_cls", [GINet, FoutNet])
def test_eval_runner_runs_twice_without_a_sync(model_cls):
    store = _store()
    torch.manual_seed(31)
    model = (GINet(30, 1, 3) if model_cls is GINet else FoutNet(30, 1)).to(DEV).eval()
    assert eval_eligible(model, store)
    runner = EvalRunner(model, store, SIZES)
    got = [runner.run(bs).clone() for bs in (B1, B2)]  # no synchronize in between
    with torch.no_grad():
        for bs, out in zip((B1, B2), got):
            ref = torch.cat([model(_Handle(BatchHandle(store, np.asarray(b, np.int32)))) for b in bs])
            assert ref.shape == (11, 1) and bool(torch.isfinite(ref).all())
            assert torch.equal(out, ref)
    assert not torch.equal(got[0], got[1])  # (the two runs do predict different orders)


def test_epoch_runner_first_use_rolls_warmup_and_capture_back_once():
    """The first ``run`` steps three times eagerly (warm-up), three times under
    capture, puts the state back and replays: afterwards everything equals a
    twin that took the three batches eagerly, once.  The second ``run`` only
    replays."""
    store = _store()
    torch.manual_seed(32)
    model = GINet(30, 1, 3).to(DEV).train()
    model._drop_seed = 4242  # noqa: SLF001
    twin = copy.deepcopy(model)
    step, ref = FusedTrainStep(model, max_batch=4), FusedTrainStep(twin, max_batch=4)
    assert eligible(step, store)
    start = [p.detach().clone() for p in step.params]
    runner = EpochRunner(step, store, SIZES)
    for epoch, bs in enumerate((B1, B2), start=1):
        loss, out = runner.run(bs)
        want = []
        for b in bs:  # (a step returns views of its buffers: cloned before the next one)
            lo, o = ref.step(BatchHandle(store, np.asarray(b, np.int32)))
            want.append((lo.clone(), o.clone()))
        assert torch.equal(loss, torch.cat([lo for lo, _ in want])), epoch
        assert torch.equal(out, torch.cat([o for _, o in want])), epoch
        assert bool(torch.isfinite(loss).all())
        assert step.step_count == ref.step_count == 3 * epoch
        assert torch.equal(step.counter, ref.counter) and int(step.counter[0].item()) == 3 * epoch
        for p, q in zip(step.params, ref.params):
            assert torch.equal(p, q), epoch
        for (m, v), (rm, rv) in zip(step.states, ref.states):
            assert torch.equal(m, rm) and torch.equal(v, rv), epoch
    assert any(not torch.equal(p, q) for p, q in zip(step.params, start))  # (the steps did train)
