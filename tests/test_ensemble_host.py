"""Host side of the multi-member training step (``deeprank2_amd.ensemble``):
the pure index helpers, the argument checks ``dr_ginet_multi_pass`` and
``dr_reduce_multi_build`` / ``dr_reduce_update_multi`` make before their first
device call, and the constructor's refusals.  No GPU needed."""

from __future__ import annotations

import ctypes

import numpy as np
import pytest
import torch

from deeprank2_amd import _lib
from deeprank2_amd.ensemble import FusedEnsembleStep, epoch_batches, kfold_indices
from deeprank2_amd.neuralnets.gnn.foutnet import FoutNet
from deeprank2_amd.neuralnets.gnn.ginet import GINet

DR_OK, DR_E_ARG, DR_E_UNSUPPORTED = 0, -1, -3


# ---- kfold_indices / epoch_batches ----------------------------------------
@pytest.mark.parametrize(("n", "k"), [(24, 3), (25, 3), (26, 4), (7, 7), (10, 1), (100, 8)])
def test_kfold_partitions_the_range(n, k):
    folds = kfold_indices(n, k, seed=11)
    assert len(folds) == k
    vals = [v for _, v in folds]
    assert np.array_equal(np.sort(np.concatenate(vals)), np.arange(n)), "the validation parts partition range(n)"
    sizes = [len(v) for v in vals]
    assert max(sizes) - min(sizes) <= 1
    for tr, va in folds:
        assert not np.intersect1d(tr, va).size
        assert np.array_equal(np.sort(np.concatenate([tr, va])), np.arange(n))


def test_kfold_is_deterministic_in_seed():
    a, b, c = kfold_indices(40, 4, 5), kfold_indices(40, 4, 5), kfold_indices(40, 4, 6)
    for (t1, v1), (t2, v2) in zip(a, b):
        assert np.array_equal(t1, t2) and np.array_equal(v1, v2)
    assert any(not np.array_equal(v1, v3) for (_, v1), (_, v3) in zip(a, c))
    with pytest.raises(ValueError, match="k must be"):
        kfold_indices(3, 4, 0)


@pytest.mark.parametrize("shuffle", [True, False])
@pytest.mark.parametrize(("n", "bs"), [(24, 5), (16, 5), (10, 5), (3, 5), (0, 5)])
def test_epoch_batches_cover_the_indices_once(n, bs, shuffle):
    idx = np.arange(100, 100 + n) * 3
    b = epoch_batches(idx, bs, shuffle, seed=1, member=2, epoch=3)
    assert len(b) == -(-n // bs)
    assert all(len(x) == bs for x in b[:-1]) and all(0 < len(x) <= bs for x in b)
    flat = np.concatenate(b) if b else np.empty(0, np.int64)
    assert np.array_equal(np.sort(flat), idx)
    if not shuffle:
        assert np.array_equal(flat, idx)


def test_epoch_batches_order_depends_on_seed_member_and_epoch():
    idx = np.arange(50)
    cat = lambda *a: np.concatenate(epoch_batches(idx, 8, True, *a))  # noqa: E731
    base = cat(3, 1, 0)
    assert np.array_equal(base, cat(3, 1, 0))
    assert np.array_equal(base, idx[np.random.default_rng([3, 1, 0]).permutation(50)])
    for other in [(3, 2, 0), (3, 1, 1), (4, 1, 0)]:
        assert not np.array_equal(base, cat(*other)), other


# ---- dr_ginet_multi_pass: checks before any launch -------------------------
def _store():
    st = _lib.GraphStoreC()
    st.n_feat, st.x_stride, st.n_edge_feat = 30, 32, 3
    return st


def _pass(**kw):
    p = _lib.PassC()
    p.flags = _lib.DR_PASS_FORWARD | _lib.DR_PASS_BACKWARD
    p.out_dim = 1
    p.loss_kind = _lib.DR_LOSS_MSE
    d = 16  # never dereferenced: the checks return first
    p.out, p.slab, p.head, p.loss_per_graph = d, d, d, d
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _members(passes, n_batch=8, weights=None):
    """(array, the objects it points to) for one member per pass struct."""
    ws = [weights or _lib.GinetWeightsC() for _ in passes]
    arr = (_lib.GinetMemberC * max(1, len(passes)))()
    for m, w, p in zip(arr, ws, passes):
        m.w, m.pass_, m.descs, m.n_batch = ctypes.pointer(w), ctypes.pointer(p), 16, n_batch
    return arr, (ws, passes)


def _multi(arr, n, st=None):
    st = st or _store()
    return _lib.load().dr_ginet_multi_pass(ctypes.byref(st), arr, n, 1024, None, 0, None)


def test_multi_pass_refuses_bad_member_counts_and_null_fields():
    arr, _keep = _members([_pass() for _ in range(8)])
    assert _multi(arr, 0) == DR_E_ARG
    assert _multi(arr, 9) == DR_E_ARG
    assert _multi(arr, -1) == DR_E_ARG
    assert _lib.load().dr_ginet_multi_pass(ctypes.byref(_store()), None, 1, 1024, None, 0, None) == DR_E_ARG
    assert _lib.load().dr_ginet_multi_pass(None, arr, 1, 1024, None, 0, None) == DR_E_ARG
    for field in ("w", "pass_", "descs"):
        arr, _keep = _members([_pass() for _ in range(3)])
        setattr(arr[1], field, None)
        assert _multi(arr, 3) == DR_E_ARG, field
    arr, _keep = _members([_pass() for _ in range(2)])
    arr[1].n_batch = -1
    assert _multi(arr, 2) == DR_E_ARG


@pytest.mark.parametrize(("loss_kind", "loss_param"), [(6, 1.0), (-1, 1.0), (_lib.DR_LOSS_HUBER, 0.0), (_lib.DR_LOSS_SMOOTH_L1, float("nan"))])
def test_multi_pass_checks_the_loss_of_every_member(loss_kind, loss_param):
    passes = [_pass(), _pass(), _pass(loss_kind=loss_kind, loss_param=loss_param)]
    arr, _keep = _members(passes, n_batch=0)  # (empty batches: the checks run all the same, and nothing is launched)
    assert _multi(arr, 3) == DR_E_ARG
    assert _multi(arr, 2) == DR_OK, "the first two members alone are fine"
    arr, _keep = _members(passes)
    assert _multi(arr, 3) == DR_E_ARG


def test_multi_pass_refuses_bf16_a_slot_and_mixed_out_dim():
    for bad in (_pass(compute_dtype=_lib.DR_DTYPE_BF16), _pass(slot=16), _pass(out_dim=2)):
        arr, _keep = _members([_pass(), bad])
        assert _multi(arr, 2) == DR_E_UNSUPPORTED
    arr, _keep = _members([_pass(), _pass(slab=None)])  # a backward pass without its partial buffers
    assert _multi(arr, 2) == DR_E_ARG
    arr, _keep = _members([_pass(), _pass()])
    assert _lib.load().dr_ginet_multi_pass(ctypes.byref(_store()), arr, 2, 161 * 1024, None, 0, None) == -2  # DR_E_LDS
    # a Z array narrower than the kernel's K, or with an odd stride
    for zs in (30, 33):
        assert _lib.load().dr_ginet_multi_pass(ctypes.byref(_store()), arr, 2, 1024, 16, zs, None) == DR_E_ARG


def test_multi_pass_with_every_batch_empty_launches_nothing():
    for n in (1, 3, 8):
        arr, _keep = _members([_pass() for _ in range(n)], n_batch=0)
        assert _multi(arr, n) == DR_OK  # (no device, no store arrays: a launch could not have succeeded)


def test_member_struct_layouts():
    assert _lib.DR_MAX_MEMBERS == 8
    assert ctypes.sizeof(_lib.GinetMemberC) == 3 * 8 + 8
    assert ctypes.sizeof(_lib.ReduceMemberC) == 5 * 8 + 8 + ctypes.sizeof(_lib.OptimC)
    # eight members by value fit the 4 KB kernel-argument segment next to the store
    assert ctypes.sizeof(_lib.GraphStoreC) + 16 + 8 * (ctypes.sizeof(_lib.GinetWeightsC) + ctypes.sizeof(_lib.PassC) + 16) <= 4096 - 256


# ---- dr_reduce_multi_build / dr_reduce_update_multi ------------------------
def _table(numel=(70, 5)):
    t = _lib.ParamTableC()
    t.n_params = len(numel)
    for i, n in enumerate(numel):
        t.param[i], t.grad[i], t.exp_avg[i], t.exp_avg_sq[i], t.numel[i] = 64, 64, 64, 64, n
        t.recipe[i].kind = _lib.DR_GRAD_SLAB
    t.slab_stride, t.head_stride, t.slab_rows = 128, 8, 1
    return t


def _reduce_members(tables, kind=_lib.DR_OPT_ADAM, n_batch=4):
    arr = (_lib.ReduceMemberC * len(tables))()
    for m, t in zip(arr, tables):
        m.t = ctypes.pointer(t) if t is not None else None
        m.slab, m.head, m.loss_per_graph, m.loss_out = 64, 64, 64, 64
        m.n_batch, m.loss_scale = n_batch, 0.25
        a = _lib.AdamC()
        a.lr, a.beta1, a.beta2, a.eps, a.enabled = 1e-3, 0.9, 0.999, 1e-8, 1
        m.opt = _lib.OptimC(a, kind, 0.0, 0.0, 0)
    return arr


def test_reduce_multi_args_bytes_is_monotonic_in_members():
    lib = _lib.load()
    sizes = [lib.dr_reduce_multi_args_bytes(k) for k in range(1, 9)]
    assert all(b > a > 0 for a, b in zip(sizes, sizes[1:]))
    assert len({b - a for a, b in zip(sizes, sizes[1:])}) == 1 and sizes[0] % 64 == 0
    assert lib.dr_reduce_multi_args_bytes(0) == -1 and lib.dr_reduce_multi_args_bytes(9) == -1


def test_reduce_multi_build_checks_and_fills():
    lib = _lib.load()
    tables = [_table(), _table(), _table()]
    arr = _reduce_members(tables)
    nbytes = lib.dr_reduce_multi_args_bytes(3)
    buf = np.zeros(nbytes, np.uint8)
    blocks = lib.dr_reduce_multi_build(arr, 3, buf.ctypes.data, nbytes)
    assert blocks == 2 + 1  # ceil(70 / 64) + ceil(5 / 64)
    assert buf.any()
    head = buf[:12].view(np.int32)
    assert tuple(head) == (3, 3, _lib.DR_OPT_ADAM)
    # the same members again give the same bytes; another batch size gives others
    again = np.zeros(nbytes, np.uint8)
    assert lib.dr_reduce_multi_build(arr, 3, again.ctypes.data, nbytes) == blocks and np.array_equal(buf, again)
    arr[1].n_batch = 0
    assert lib.dr_reduce_multi_build(arr, 3, again.ctypes.data, nbytes) == blocks and not np.array_equal(buf, again)
    # refusals leave the buffer as it was
    keep = again.copy()
    assert lib.dr_reduce_multi_build(arr, 3, again.ctypes.data, nbytes - 1) == DR_E_ARG  # a short buffer
    assert lib.dr_reduce_multi_build(arr, 0, again.ctypes.data, nbytes) == DR_E_ARG
    assert lib.dr_reduce_multi_build(arr, 9, again.ctypes.data, 1 << 20) == DR_E_ARG
    assert lib.dr_reduce_multi_build(None, 3, again.ctypes.data, nbytes) == DR_E_ARG
    assert lib.dr_reduce_multi_build(arr, 3, None, nbytes) == DR_E_ARG
    assert lib.dr_reduce_multi_build(_reduce_members([_table(), None, _table()]), 3, again.ctypes.data, nbytes) == DR_E_ARG  # a null table
    t_null = _table()
    t_null.param[1] = None
    assert lib.dr_reduce_multi_build(_reduce_members([_table(), t_null]), 2, again.ctypes.data, nbytes) == DR_E_ARG
    assert lib.dr_reduce_multi_build(_reduce_members([_table(), _table((70, 6))]), 2, again.ctypes.data, nbytes) == DR_E_ARG  # another architecture
    mixed = _reduce_members([_table(), _table()])
    mixed[1].opt.kind = _lib.DR_OPT_ADAMAX
    assert lib.dr_reduce_multi_build(mixed, 2, again.ctypes.data, nbytes) == DR_E_ARG  # one rule per launch
    assert lib.dr_reduce_multi_build(_reduce_members([_table()], kind=3), 1, again.ctypes.data, nbytes) == DR_E_ARG
    assert np.array_equal(keep, again)


def test_reduce_update_multi_argument_checks_are_host_only():
    lib = _lib.load()
    d = 64
    assert lib.dr_reduce_update_multi(None, 2, 3, 0, None) == DR_E_ARG
    assert lib.dr_reduce_update_multi(d + 4, 2, 3, 0, None) == DR_E_ARG  # not 64-byte aligned
    for k in (0, 9):
        assert lib.dr_reduce_update_multi(d, k, 3, 0, None) == DR_E_ARG
    assert lib.dr_reduce_update_multi(d, 2, -1, 0, None) == DR_E_ARG
    assert lib.dr_reduce_update_multi(d, 2, 513, 0, None) == DR_E_ARG
    assert lib.dr_reduce_update_multi(d, 2, 3, 3, None) == DR_E_ARG
    assert lib.dr_reduce_update_multi(d, 2, 0, 0, None) == DR_OK  # nothing to do, nothing launched


# ---- FusedEnsembleStep: refusals that come before any device work ----------
def test_ensemble_step_refuses_what_it_cannot_run():
    torch.manual_seed(0)
    g = lambda f=30, out=1: GINet(f, out, 3)  # noqa: E731
    with pytest.raises(ValueError, match="1 to 8 members"):
        FusedEnsembleStep([g() for _ in range(9)])
    with pytest.raises(ValueError, match="1 to 8 members"):
        FusedEnsembleStep([])
    with pytest.raises(ValueError, match="input_shape"):
        FusedEnsembleStep([g(30), g(33)])
    with pytest.raises(ValueError, match="input_shape"):
        FusedEnsembleStep([g(30, 1), g(30, 2)])
    with pytest.raises(ValueError, match="GINet"):
        FusedEnsembleStep([g(), FoutNet(30, 1)])
    with pytest.raises(ValueError, match="fp32"):
        FusedEnsembleStep([g(), g()], compute_dtype="bf16")
    with pytest.raises(ValueError, match="single-device"):
        FusedEnsembleStep([g(), g()], process_group=object())
    with pytest.raises(ValueError, match="lr has 3 entries"):
        FusedEnsembleStep([g(), g()], lr=[1e-3, 2e-3, 3e-3])
    m = g()
    with pytest.raises(ValueError, match="distinct"):
        FusedEnsembleStep([m, m])
