"""GINet's conv1 neighbour sums built once per store (``GraphStore.agg_x``,
``dr_aggregate_x``) and the kernels that read them instead of gathering
(``dr_ginet_graph_pass_z`` / ``dr_ginet_acc_pass_z``).

``Z = A x`` depends only on the store's ``x`` and CSR, so nothing here has a
tolerance:

* ``agg_x()`` equals a numpy float32 sum over each CSR row, one add per edge in
  CSR order from +0 (the kernels' own gather order), bit for bit, with exact
  zeros in the columns past F and in the stride padding;
* a pass through the Z-input kernels equals the same pass through the gather
  entries in every output (``torch.equal``): per-graph kernel and accumulating
  pass, both of its layouts, eager and replayed from a captured graph;
* switched off, no Z array is ever allocated.
"""

from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

from deeprank2_amd import _lib
from deeprank2_amd.engine import FusedTrainStep
from deeprank2_amd.fused import LDS_MAX, BatchHandle, Dropout, lds_for
from deeprank2_amd.neuralnets.gnn import ginet as amd
from deeprank2_amd.store import GraphRecord, GraphStore, pack_graphs
from deeprank2_amd.utils.synthetic import doubled_edges, make_dataset

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FWD, BWD = _lib.DR_PASS_FORWARD, _lib.DR_PASS_BACKWARD


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
    """The graphs of the issue's list, F = ``f`` (a tuple of records, by position):
    0 a 17-node residue graph (odd N, so every later block starts at an odd
    node offset); 1 one node; 2 twenty nodes and no edge; 3-6 N = 15, 16, 17,
    33 (tile edges); 7 a row with a repeated neighbour (0 -> 1 three times,
    between other edges); 8 a directed ring with chords (asymmetric: the store's
    transpose is not aliased); 9, 10 two ~60-node residue graphs with two
    depth-1 clusters."""
    rng = np.random.default_rng(77 + f)
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


def _z_reference(packed):
    """Z = A x by float32 adds, one per edge in CSR order from +0, per graph."""
    z = np.zeros((packed.x.shape[0], packed.n_feat), np.float32)
    for g in range(packed.n_graphs):
        n0, n1 = int(packed.node_off[g]), int(packed.node_off[g + 1])
        e0, e1 = int(packed.edge_off[g]), int(packed.edge_off[g + 1])
        rp, col, x = packed.rowptr[n0 + g : n1 + g + 1], packed.col[e0:e1].astype(np.int64), packed.x[n0:n1].astype(np.float32)
        for i in range(n1 - n0):
            acc = np.zeros(packed.n_feat, np.float32)
            for e in range(int(rp[i]), int(rp[i + 1])):
                acc = acc + x[col[e]]  # float32 + float32, elementwise: one rounding per add
            z[n0 + i] = acc
    return z


@pytest.mark.parametrize("f", [1, 12, 30, 33, 64])
def test_agg_x_is_the_csr_order_sum_bit_for_bit(f):
    """Both K paddings (32 for F <= 32, else 64), F not a multiple of 4, and
    every graph of ``_zoo``: the graph under test is never the store's only or
    first one, and the blocks after graph 0 start at odd node offsets."""
    packed = _zoo_packed(f)
    assert int(packed.transpose_aliased) == 0 and packed.node_off[1] % 2 == 1
    store = GraphStore(packed, DEV)
    z = store.agg_x()
    torch.cuda.synchronize()
    stride = store.agg_x_stride
    assert stride >= (32 if f <= 32 else 64) and z.shape == (packed.x.shape[0], stride) and z.dtype == torch.float32
    assert store.agg_x() is z, "built once, then cached"
    got = z.cpu().numpy()
    ref = _z_reference(packed)
    assert np.array_equal(got[:, :f].view(np.uint32), ref.view(np.uint32)), "Z differs from the CSR-order float32 sum"
    assert not got[:, f:].view(np.uint32).any(), "columns past F and the stride padding must be +0"
    n0 = int(packed.node_off[2])
    assert not got[n0 : n0 + 20].view(np.uint32).any(), "a graph without edges has Z = +0"


def _run_pass(store, gids, params, out_dim, flags, loss_kind, dropout, use_z):
    """One graph pass; every output the pass can write, from zero-filled buffers."""
    store.use_agg_x = use_z
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


@pytest.mark.parametrize("f", [30, 40])
@pytest.mark.parametrize("flags", [FWD, FWD | BWD], ids=["fwd", "fwd_bwd"])
@pytest.mark.parametrize("loss", ["mse_dropout", "ce2"])
def test_pass_through_z_equals_pass_through_gather(f, flags, loss):
    """B = 8: one node, no edges, N = 16 and 33, the repeated-neighbour row,
    the asymmetric ring and the two ~60-node graphs with K1 = 2, in a shuffled
    order, on both kernels' K (F = 30, 40)."""
    packed = _zoo_packed(f)
    store = GraphStore(packed, DEV)
    gids = [9, 1, 4, 7, 10, 2, 8, 6]
    out_dim = 1 if loss == "mse_dropout" else 2
    if out_dim == 2:  # noqa: PLR2004
        store.set_targets(np.arange(packed.n_graphs) % 2)
    torch.manual_seed(3)
    params = amd.GINet(f, out_dim, 3).to(DEV).ordered_params()
    kind = _lib.DR_LOSS_MSE if out_dim == 1 else _lib.DR_LOSS_CE
    drop = Dropout(0.4, seed=12345, offset=7) if loss == "mse_dropout" else None
    new = _run_pass(store, gids, params, out_dim, flags, kind, drop, use_z=True)
    assert store._agg_x is not None, "the Z-input entry was not taken"  # noqa: SLF001
    old = _run_pass(store, gids, params, out_dim, flags, kind, drop, use_z=False)
    for name in new:
        assert torch.equal(new[name], old[name]), name
    assert bool(new["out"].abs().sum() > 0)
    if flags & BWD:
        assert bool(new["slab"].abs().sum() > 0) and bool(new["head"].abs().sum() > 0)


@functools.lru_cache(maxsize=None)
def _ragged_packed(f):
    """40 residue graphs of 30 to 210 nodes (F = 40: to 120, so both layouts,
    with 64-wide rows and the LDS fc1.weight sums, fit one workgroup)."""
    return pack_graphs(_syn(40, 41, f, n_lo=30, n_hi=210 if f <= 32 else 120))  # noqa: PLR2004


def _trainer(f, seed=5, **attrs):
    torch.manual_seed(seed)
    m = amd.GINet(f, 1, 3).to(DEV).train()
    m._drop_seed = 777  # noqa: SLF001
    step = FusedTrainStep(m, loss="mse", max_batch=64)
    for k, v in attrs.items():
        setattr(step, k, v)
    return step


@pytest.mark.parametrize(("groups", "prefetch", "f"), [(1, True, 30), (1, False, 30), (7, True, 30), (7, False, 30), (7, True, 40), (7, False, 40)])
def test_acc_pass_through_z_equals_acc_pass_through_gather(groups, prefetch, f):
    """B = 40 on 1 and on 7 workgroups, prefetch layout on and off: the same
    per-graph arithmetic in the same summation order, so the partial rows, the
    outputs, the loss and the updated state are equal, not close."""
    res = []
    for use_z in (True, False):
        store = GraphStore(_ragged_packed(f), DEV)
        store.use_agg_x = use_z
        step = _trainer(f, acc=True, acc_groups=groups, acc_prefetch=prefetch)
        h = BatchHandle(store, np.arange(40, dtype=np.int32))
        assert step._acc_rows(h) == groups  # noqa: SLF001
        pf_bytes = int(_lib.load().dr_ginet_acc_lds_bytes(step._acc_max_sizes(h), f, int(store.packed.transpose_aliased), 1)) if prefetch else -1  # noqa: SLF001
        assert (0 < pf_bytes <= LDS_MAX) == prefetch, "the layout under test must be the one taken"
        loss, out = step.step(h)
        torch.cuda.synchronize()
        assert (store._agg_x is not None) == use_z  # noqa: SLF001
        rs = int(_lib.load().dr_ginet_acc_row_floats(f, 1))
        # (a row's written part: the stride rounds it up to 16 bytes, the pad is never written)
        rows = step._acc_slab[: groups * rs].view(groups, rs)[:, : 32 * f + 1024 + 128 * 64 + 128 + 128 + 1]  # noqa: SLF001
        res.append((loss.clone(), out.clone(), rows.clone(), [t.clone() for t in step._state_tensors()]))  # noqa: SLF001
    (l1, o1, r1, s1), (l2, o2, r2, s2) = res
    assert torch.equal(o1, o2), "outputs"
    assert torch.equal(l1, l2), "loss"
    assert torch.equal(r1, r2), "partial rows"
    assert bool(r1.abs().sum() > 0)
    for k, (a, b) in enumerate(zip(s1, s2)):
        assert torch.equal(a, b), f"state tensor {k}"


def test_acc_pass_small_f_where_the_z_prefetch_layout_does_not_fit():
    """F = 4, N = 470-480, E ~ 15 N, three graphs per workgroup.  The prefetch
    layout keeps its inputs once per parity: x, rowptr and col in the gather
    form (2 (4 N + N + E / 2) words, plus Z once, 34 N), Z itself in the Z form
    (2 * 36 N words).  Here the gather form's layout fits 160 KiB, so the
    accumulating pass is taken with prefetch, and the Z form's does not: the
    Z-input entry must then run without prefetch (its plain carve fits) and
    give the gather entry's results, not refuse the batch."""
    f, rng = 4, np.random.default_rng(8)
    recs = _syn(6, 43, f, n_lo=470, n_hi=480, mean_degree=15.0, kd_min_nodes=10**9)
    for r in recs:  # (the synthetic x's first four columns are one-hot flags)
        r.x = rng.normal(size=r.x.shape).astype(np.float32)
    packed = pack_graphs(recs)
    lib, r4 = _lib.load(), lambda v: (v + 3) & ~3
    res = []
    for use_z in (True, False):
        store = GraphStore(packed, DEV)
        store.use_agg_x = use_z
        step = _trainer(f, acc=True, acc_groups=2, acc_prefetch=True)
        h = BatchHandle(store, np.arange(6, dtype=np.int32))
        assert step._acc_rows(h) == 2  # noqa: SLF001
        n, e, k0, p1, k1 = h.max_sizes
        alias = int(packed.transpose_aliased)
        pf_gather = int(lib.dr_ginet_acc_lds_bytes(step._acc_max_sizes(h), f, alias, 1))  # noqa: SLF001
        # the Z form's layout: per parity r4(36 N) for r4(r4(F) N) + r4(N + 1) + r4((E + 1) / 2), and no Z in the scratch
        pf_z = pf_gather + 4 * (2 * (r4(36 * n) - r4(r4(f) * n) - r4(n + 1) - r4((e + 1) // 2)) - r4(34 * n))
        acc_words = 32 * f + 1024 + r4(128 + 128 + 1 + 1) + 4
        plain_z = int(lib.dr_ginet_z_lds_bytes(n, e, f, k0, p1, k1, alias, 1, store.agg_x_stride)) + 4 * acc_words
        assert 0 < pf_gather <= LDS_MAX < pf_z and plain_z <= LDS_MAX, (pf_gather, pf_z, plain_z)
        loss, out = step.step(h)
        torch.cuda.synchronize()
        assert (store._agg_x is not None) == use_z  # noqa: SLF001
        rs = int(lib.dr_ginet_acc_row_floats(f, 1))
        rows = step._acc_slab[: 2 * rs].view(2, rs)[:, : 32 * f + 1024 + 128 * 64 + 128 + 128 + 1]  # noqa: SLF001
        res.append((loss.clone(), out.clone(), rows.clone(), [t.clone() for t in step._state_tensors()]))  # noqa: SLF001
    (l1, o1, r1, s1), (l2, o2, r2, s2) = res
    assert torch.equal(o1, o2) and torch.equal(l1, l2) and torch.equal(r1, r2)
    assert bool(r1.abs().sum() > 0) and bool(torch.isfinite(l1).all())
    for k, (a, b) in enumerate(zip(s1, s2)):
        assert torch.equal(a, b), f"state tensor {k}"


def test_captured_steps_equal_eager_steps_with_z():
    """Three replays of one captured step equal three eager steps, bit for bit."""
    store = GraphStore(_zoo_packed(30), DEV)
    h = BatchHandle(store, np.asarray([9, 1, 4, 7, 10, 2, 8, 6], np.int32))
    one, two = _trainer(30), _trainer(30)
    g = one.capture(h)
    assert store._agg_x is not None  # noqa: SLF001
    for _ in range(3):
        g.replay()
        two.step(h)
    torch.cuda.synchronize()
    for k, (a, b) in enumerate(zip(one._state_tensors(), two._state_tensors())):  # noqa: SLF001
        assert torch.equal(a, b), f"state tensor {k}"


def test_capture_on_a_fresh_store_builds_z_in_its_warm_up():
    """No eager step of the test's own before the capture: the capture's eager
    warm-up builds Z (nothing is allocated while capturing), the captured step
    reads it, and a replay equals an eager step through the gather entry."""
    fresh, plain = GraphStore(_zoo_packed(30), DEV), GraphStore(_zoo_packed(30), DEV)
    plain.use_agg_x = False
    gids = np.asarray([10, 3, 8, 0, 9, 7], np.int32)
    one, two = _trainer(30), _trainer(30)
    assert fresh._agg_x is None  # noqa: SLF001
    g = one.capture(BatchHandle(fresh, gids))
    assert fresh._agg_x is not None  # noqa: SLF001
    g.replay()
    two.step(BatchHandle(plain, gids))
    torch.cuda.synchronize()
    assert plain._agg_x is None  # noqa: SLF001
    for k, (a, b) in enumerate(zip(one._state_tensors(), two._state_tensors())):  # noqa: SLF001
        assert torch.equal(a, b), f"state tensor {k}"
    assert torch.equal(one.out[: len(gids)], two.out[: len(gids)])


@pytest.mark.parametrize("how", ["env", "attribute"])
def test_switched_off_no_z_is_allocated(how, monkeypatch):
    if how == "env":  # (read once, when the store is made)
        monkeypatch.setenv("DR_GINET_AGGX", "0")
    store = GraphStore(_zoo_packed(30), DEV)
    if how == "attribute":
        store.use_agg_x = False
    step = _trainer(30)
    h = BatchHandle(store, np.arange(store.n_graphs, dtype=np.int32))
    step.step(h)
    step.acc, step.acc_groups = True, 3
    step.step(h)
    torch.cuda.synchronize()
    assert store.agg_x() is None and store._agg_x is None  # noqa: SLF001
