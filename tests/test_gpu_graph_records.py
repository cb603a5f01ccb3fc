"""One record per graph (``GraphStore.graph_records``, ``dr_graph_records``) and
the passes that stage a graph from it by one linear copy
(``dr_ginet_graph_pass_rec`` / ``dr_ginet_acc_pass_rec``).

No arithmetic moves, so nothing here has a tolerance:

* every section of every record is ``torch.equal`` to the rows of ``agg_x()``
  and to the store arrays' slices, with zero padding;
* a pass through the record entry equals the pass through the Z-input entry
  and through the gather entry in every output;
* the accumulating pass's rows are equal, with and without the prefetch layout;
* three replays of a captured step leave the state the Z-input run leaves.

Five graphs, chosen for the layout: one node and no edge (K0 = K1 = 1); N = 16
and N = 17 (the tile edge); N = 33 with 17 depth-0 clusters (the other pooling
path) in two depth-1 clusters; and a directed ring with chords, which makes the
store's pooled transpose a copy of its own (not aliased).
"""

from __future__ import annotations

import functools

import numpy as np
import pytest
import torch
from test_gpu_aggx import _hand, _syn, _trainer

from deeprank2_amd import _lib
from deeprank2_amd.fused import LDS_MAX, BatchHandle, Dropout, lds_for
from deeprank2_amd.neuralnets.gnn import ginet as amd
from deeprank2_amd.store import GraphStore, pack_graphs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FWD, BWD = _lib.DR_PASS_FORWARD, _lib.DR_PASS_BACKWARD
MODES = {"rec": (True, True), "z": (True, False), "gather": (False, False)}  # use_agg_x, use_records


@functools.lru_cache(maxsize=None)
def _packed(f, aliased):
    rng = np.random.default_rng(31 + f)
    recs = [_hand(rng, 1, f, [], [0], [0], "one_node")]
    for n in (16, 17):
        recs += _syn(1, 600 + n, f, n_lo=n, n_hi=n, mean_degree=6.0, k_lo=2, k_hi=5)
    big = _syn(1, 633, f, n_lo=33, n_hi=33, mean_degree=6.0, k_lo=2, k_hi=5)[0]
    big.cluster0 = np.arange(33, dtype=np.int64) % 17
    big.cluster1 = np.arange(17, dtype=np.int64) % 2
    recs.append(big)
    if not aliased:
        ring = np.arange(24)
        recs.append(_hand(rng, 24, f, np.concatenate([np.stack([ring, (ring + 1) % 24], 1), np.stack([ring, (ring + 5) % 24], 1)]), ring % 6, np.arange(6) % 3, "ring_chords"))
    p = pack_graphs(recs)
    assert bool(p.transpose_aliased) == aliased
    n, _, k0, _, k1 = p.sizes()
    assert n[:4].tolist() == [1, 16, 17, 33] and (k0[0], k1[0]) == (1, 1) and k0[3] == 17 and k1[3] == 2  # noqa: PLR2004
    return p


def _store(f, aliased, mode):
    store = GraphStore(_packed(f, aliased), DEV)
    store.use_agg_x, store.use_records = MODES[mode]
    return store


@pytest.mark.parametrize("aliased", [False, True], ids=["own_transpose", "aliased"])
@pytest.mark.parametrize("f", [1, 30, 32, 33])
def test_record_sections_equal_agg_x_and_the_store_arrays(f, aliased):
    store = _store(f, aliased, "rec")
    p = store.packed
    rec = store.graph_records()
    torch.cuda.synchronize()
    assert rec is not None and store.graph_records() is rec, "built once, then cached"
    z, zs = store.agg_x(), store.agg_x_stride
    n, _, k0, p1, k1 = p.sizes()
    words = rec.view(torch.int32)
    assert rec.numel() == int(store.rec_off_host[-1])
    for g in range(p.n_graphs):
        N, K0, P1, K1 = int(n[g]), int(k0[g]), int(p1[g]), int(k1[g])
        o = int(store.rec_off_host[g])
        assert o % 4 == 0

        def section(src, length, o0, g=g):
            got = words[o0 : o0 + ((length + 3) & ~3)]
            assert torch.equal(got[:length], src.view(torch.int32).reshape(-1)[:length]), g
            assert not bool(got[length:].any()), f"graph {g}: padding must be zero"
            return o0 + ((length + 3) & ~3)

        n0, q0 = int(p.node_off[g]), int(p.p1_off[g])
        kk0, kk1 = int(p.k0_off[g]), int(p.k1_off[g])
        o = section(z[n0 : n0 + N].contiguous(), N * zs, o)  # (the same bits as agg_x: compared as words)
        o = section(store.cl0[n0:], N, o)
        o = section(store.p1_rowptr[kk0 + g :], K0 + 1, o)
        o = section(store.p1_col[q0:], P1, o)
        if not aliased:
            o = section(store.p1t_rowptr[kk0 + g :], K0 + 1, o)
            o = section(store.p1t_col[q0:], P1, o)
        o = section(store.m1_ptr[kk1 + g :], K1 + 1, o)
        o = section(store.m1_idx[kk0:], K0, o)
        assert o == int(store.rec_off_host[g + 1])


def _run_pass(store, gids, params, out_dim, flags, loss_kind, dropout):
    h = BatchHandle(store, np.asarray(gids, np.int32))
    assert lds_for(amd.SPEC, h, out_dim) <= LDS_MAX
    b, f = h.B, store.n_feat
    out = torch.zeros(b, out_dim, device=DEV)
    lpg = torch.zeros(b, device=DEV)
    slab = torch.zeros(b * amd.slab_stride(f), device=DEV)
    head = torch.zeros(b * amd.head_stride(out_dim), device=DEV)
    amd.graph_pass(h, params, out_dim, flags, dropout=dropout, loss_kind=loss_kind, loss_scale=1.0 / b, out=out, loss_per_graph=lpg, slab=slab, head=head)
    torch.cuda.synchronize()
    return {"out": out, "loss_per_graph": lpg, "slab": slab, "head": head}


@pytest.mark.parametrize(("f", "aliased"), [(1, False), (30, False), (30, True), (32, False), (33, False)])
@pytest.mark.parametrize("loss", ["mse_dropout", "ce2"])
def test_pass_through_records_equals_z_and_gather(f, aliased, loss):
    """Every graph of the store in a shuffled order, forward + backward; F = 33
    runs the 64-wide kernel."""
    out_dim = 1 if loss == "mse_dropout" else 2
    kind = _lib.DR_LOSS_MSE if out_dim == 1 else _lib.DR_LOSS_CE
    drop = Dropout(0.4, seed=4321, offset=5) if loss == "mse_dropout" else None
    torch.manual_seed(3)
    params = amd.GINet(f, out_dim, 3).to(DEV).ordered_params()
    res = {}
    for mode in MODES:
        store = _store(f, aliased, mode)
        gids = [3, 0, 2, 1] if aliased else [3, 0, 4, 2, 1]
        if out_dim == 2:  # noqa: PLR2004
            store.set_targets(np.arange(store.n_graphs) % 2)
        res[mode] = _run_pass(store, gids, params, out_dim, FWD | BWD, kind, drop)
        assert (store._records is not None) == (mode == "rec"), "the entry under test was not the one taken"  # noqa: SLF001
        assert (store._agg_x is not None) == (mode != "gather")  # noqa: SLF001
    for name in res["rec"]:
        assert torch.equal(res["rec"][name], res["z"][name]), f"{name}: records against Z"
        assert torch.equal(res["rec"][name], res["gather"][name]), f"{name}: records against gather"
    assert bool(res["rec"]["out"].abs().sum() > 0) and bool(res["rec"]["slab"].abs().sum() > 0) and bool(res["rec"]["head"].abs().sum() > 0)


@pytest.mark.parametrize(("f", "prefetch"), [(30, True), (30, False), (33, True), (33, False)])
def test_acc_pass_through_records_equals_z(f, prefetch):
    """Five graphs on two workgroups (three and two graphs each, so a workgroup
    stages a next graph under the running one's tail in the prefetch layout)."""
    res = []
    for mode in ("rec", "z"):
        store = _store(f, False, mode)
        step = _trainer(f, acc=True, acc_groups=2, acc_prefetch=prefetch)
        h = BatchHandle(store, np.asarray([3, 0, 4, 2, 1], np.int32))
        assert step._acc_rows(h) == 2  # noqa: SLF001, PLR2004
        loss, out = step.step(h)
        torch.cuda.synchronize()
        assert (store._records is not None) == (mode == "rec")  # noqa: SLF001
        rs = int(_lib.load().dr_ginet_acc_row_floats(f, 1))
        rows = step._acc_slab[: 2 * rs].view(2, rs)[:, : 32 * f + 1024 + 128 * 64 + 128 + 128 + 1]  # noqa: SLF001
        res.append((loss.clone(), out.clone(), rows.clone(), [t.clone() for t in step._state_tensors()]))  # noqa: SLF001
    (l1, o1, r1, s1), (l2, o2, r2, s2) = res
    assert torch.equal(o1, o2) and torch.equal(l1, l2), "outputs, loss"
    assert torch.equal(r1, r2), "partial rows"
    assert bool(r1.abs().sum() > 0) and bool(torch.isfinite(l1).all())
    for k, (a, b) in enumerate(zip(s1, s2)):
        assert torch.equal(a, b), f"state tensor {k}"


def test_captured_steps_through_records_equal_the_z_run():
    """The capture's eager warm-up builds the records (nothing is built while
    capturing); three replays leave the state three eager Z-input steps leave."""
    gids = np.asarray([3, 0, 4, 2, 1], np.int32)
    rec_store, z_store = _store(30, False, "rec"), _store(30, False, "z")
    one, two = _trainer(30), _trainer(30)
    assert rec_store._records is None  # noqa: SLF001
    g = one.capture(BatchHandle(rec_store, gids))
    assert rec_store._records is not None  # noqa: SLF001
    hz = BatchHandle(z_store, gids)
    for _ in range(3):
        g.replay()
        two.step(hz)
    torch.cuda.synchronize()
    assert z_store._records is None and z_store._agg_x is not None  # noqa: SLF001
    for k, (a, b) in enumerate(zip(one._state_tensors(), two._state_tensors())):  # noqa: SLF001
        assert torch.equal(a, b), f"state tensor {k}"
    assert torch.equal(one.out[: len(gids)], two.out[: len(gids)])
