"""GINet's tail (``ginet_tail``: conv2 on the pooled graph, the depth-1 pooling
and its backward, dW2 / dP1, dW1, and the head) on the designed pooled graphs
of ``tail_cases.py``, every case against one **fp64** training step of the CPU
oracle, with the kernels' own hash dropout.

The tail's loops read a pooled row's neighbours in groups and end with a group
of exactly the remaining size (2 in conv2 forward, 4 in the pooling backward
and in the tie count over the K0 < 16 members of a single depth-1 cluster).
The cases put the row degrees on both sides of each group size, K0 on both sides of the tail's
switches (12 and 16), one to three depth-1 clusters, an isolated cluster and a
pooled graph whose transpose is a copy of its own
(``test_tail_cases_host.py`` proves each batch's claim).  A last group
that is one neighbour short, or runs one past the row, changes a conv2 sum or
a dY2 sum by a whole term: far outside the tolerance (builds with either
mutation fail 36 and 28 of the 38 cases).

Each case runs through the four ways a graph reaches the tail: the record
entry, the gather entry (``use_agg_x = False``), the accumulating pass (one
workgroup running both graphs) and the forced tile + tail path.  Tolerances
are ``width_cases.ratios``': outputs rtol = atol = 1e-4, loss 1e-4 relative,
gradients rtol 1e-4 with the normwise floor 1e-6.  Each run prints its largest
error as a fraction of that tolerance (``pytest -s``).
"""

from __future__ import annotations

import functools

import numpy as np
import pytest
import tail_cases as T
import torch
import width_cases as W

from deeprank2_amd.engine import FusedTrainStep
from deeprank2_amd.fused import BatchHandle
from deeprank2_amd.neuralnets.gnn import ginet
from deeprank2_amd.store import GraphStore

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PATHS = ("records", "gather", "acc", "tile_tail")


@functools.lru_cache(maxsize=None)
def _store(name, f, out, use_agg_x):
    store = GraphStore(T.packed(name, f, out), DEV)
    store.use_agg_x = use_agg_x
    return store


def _run(name, f, out, path):
    ref = T.oracle(name, f, out)
    store = _store(name, f, out, path != "gather")
    h = BatchHandle(store, np.arange(T.GRAPHS))
    if path == "tile_tail":
        h.force_large = True
    model = ginet.GINet(f, out, 3)
    model.load_state_dict(ref["state"])
    model = model.to(DEV).train()
    model._drop_seed = T.DROP_SEED  # noqa: SLF001
    step = FusedTrainStep(model, loss="mse" if out == 1 else "ce")
    step.acc, step.acc_groups = (True, 1) if path == "acc" else (False, None)
    assert int(step.counter[0]) == 0  # the hash's offset: T.keep_mask() replicates step 0
    loss, res = step.step(h)
    torch.cuda.synchronize()
    # the entry the run is about
    assert (step._acc_rows(h) > 0) == (path == "acc")  # noqa: SLF001
    assert (h._lds.get(("large", out, False, "ginet")) is not None) == (path == "tile_tail")  # noqa: SLF001
    assert (store._agg_x is not None) == (path != "gather")  # noqa: SLF001
    return {"out": res.cpu().numpy().copy(), "loss": float(loss), "grads": {n: g.cpu().numpy().copy() for n, g in zip(ginet.PARAM_NAMES, step.grads)}}


@pytest.mark.parametrize("c", T.all_cases(), ids=T.case_id)
def test_tail_on_designed_pooled_graphs_vs_fp64_oracle(c):
    name, f, out = c
    ref = T.oracle(name, f, out)
    failures = []
    for path in PATHS:
        got = _run(name, f, out, path)
        assert set(got["grads"]) == set(ref["grads"]) and got["out"].shape == ref["out"].shape
        r = W.ratios(got, ref)
        worst = max(r, key=r.get)
        print(f"[tail {T.case_id(c)} {path}] worst {worst}: {r[worst]:.3f} of the tolerance; out {r['out']:.3f} loss {r['loss']:.3f}")
        for n, g in ref["grads"].items():
            if not np.any(g):  # exact zeros stay exact (the attention's singleton softmax; K0 = 1: nothing below the head)
                assert not np.any(got["grads"][n]), f"{path}: {n}: expected exact zeros"
        failures += [f"{path}: {k} at {v:.3g} of the tolerance" for k, v in r.items() if not v <= 1.0]
    assert not failures, failures
