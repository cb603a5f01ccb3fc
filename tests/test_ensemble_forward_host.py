"""Host side of the ensemble's forward path (``deeprank2_amd.ensemble``): the
argument checks ``dr_ensemble_stats`` makes before any device work, and the
refusals of ``FusedEnsembleForward`` and ``out_of_fold_predictions`` that come
before they touch a store or a device.  No GPU needed."""

from __future__ import annotations

import ctypes

import numpy as np
import pytest
import torch

from deeprank2_amd import _lib
from deeprank2_amd.ensemble import EnsembleResult, FusedEnsembleForward, _check_batches, out_of_fold_predictions
from deeprank2_amd.neuralnets.gnn.foutnet import FoutNet
from deeprank2_amd.neuralnets.gnn.ginet import GINet

DR_OK, DR_E_ARG = 0, -1
D = 64  # a dummy pointer, never dereferenced: the checks return first


def _stats(out=D, stride=64, k=2, n=4, out_dim=2, kind=_lib.DR_ENS_CLASSIF, mean=D, spread=D, label=D):
    return _lib.load().dr_ensemble_stats(out, stride, k, n, out_dim, kind, mean, spread, label, None)


def test_ensemble_stats_is_declared_and_bound():
    assert (_lib.DR_ENS_REGRESS, _lib.DR_ENS_CLASSIF) == (0, 1)
    sig = {n: (r, a) for n, r, a in _lib.SIGNATURES}["dr_ensemble_stats"]
    assert sig[0] is ctypes.c_int and len(sig[1]) == 10 and sig[1][1] is ctypes.c_int64


@pytest.mark.parametrize(
    "bad",
    [
        dict(out=None),
        dict(mean=None),
        dict(spread=None),
        dict(label=None),  # classification writes labels
        dict(k=0),
        dict(k=-1),
        dict(k=_lib.DR_MAX_MEMBERS + 1),
        dict(out_dim=0),
        dict(out_dim=_lib.DR_MAX_OUT + 1),
        dict(n=-1),
        dict(stride=7),  # n * out_dim = 8 floats per member
        dict(stride=-64),
        dict(kind=2),
        dict(kind=-1),
    ],
    ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()),
)
def test_ensemble_stats_refuses_before_any_device_work(bad):
    assert _stats(**bad) == DR_E_ARG
    if "label" not in bad and "kind" not in bad:
        assert _stats(**bad, kind=_lib.DR_ENS_REGRESS) == DR_E_ARG


def test_ensemble_stats_with_no_graph_launches_nothing():
    for kind in (_lib.DR_ENS_REGRESS, _lib.DR_ENS_CLASSIF):
        for k in (1, 2, _lib.DR_MAX_MEMBERS):
            for out_dim in (1, _lib.DR_MAX_OUT):
                assert _stats(k=k, n=0, out_dim=out_dim, kind=kind, stride=0) == DR_OK  # (no device: a launch could not have succeeded)
    assert _stats(n=0, kind=_lib.DR_ENS_REGRESS, label=None) == DR_OK  # regression takes no label
    # the refusals hold for an empty input too
    assert _stats(n=0, k=9) == DR_E_ARG and _stats(n=0, kind=5) == DR_E_ARG and _stats(n=0, label=None) == DR_E_ARG


def test_ensemble_stats_stride_rule_is_for_several_members_only():
    # one member: the stride is never used; it is checked in 64 bits against n * out_dim
    assert _stats(k=1, n=0, stride=0) == DR_OK
    assert _stats(k=2, n=(1 << 30), out_dim=16, stride=(1 << 34) - 1) == DR_E_ARG


def _g(f=30, out=1):
    return GINet(f, out, 3)


def test_forward_runner_refuses_what_it_cannot_run():
    torch.manual_seed(0)
    with pytest.raises(ValueError, match="1 to 8 members"):
        FusedEnsembleForward([], None, [])
    with pytest.raises(ValueError, match="1 to 8 members"):
        FusedEnsembleForward([_g() for _ in range(9)], None, [[4]] * 9)
    with pytest.raises(ValueError, match="GINet"):
        FusedEnsembleForward([_g(), FoutNet(30, 1)], None, [[4], [4]])
    with pytest.raises(ValueError, match="input_shape"):
        FusedEnsembleForward([_g(30), _g(33)], None, [[4], [4]])
    with pytest.raises(ValueError, match="input_shape"):
        FusedEnsembleForward([_g(30, 1), _g(30, 2)], None, [[4], [4]])
    m = _g()
    with pytest.raises(ValueError, match="distinct"):
        FusedEnsembleForward([m, m], None, [[4], [4]])
    with pytest.raises(ValueError, match="sizes has 3 entries for 2 members"):
        FusedEnsembleForward([_g(), _g()], None, [[4], [4], [4]])
    with pytest.raises(ValueError, match="positive"):
        FusedEnsembleForward([_g(), _g()], None, [[4, 0], [4]])
    with pytest.raises(ValueError, match="cuda"):  # no CPU fallback
        FusedEnsembleForward([_g(), _g()], None, [[4], [4]])


def test_run_batches_must_match_the_sizes():
    """The check ``FusedEnsembleForward.run`` makes first, on the host."""
    sizes = [[4, 2], [3]]
    ok = [[np.arange(4), np.arange(2)], [[5, 6, 7]]]
    got = _check_batches(sizes, ok, n_graphs=8)
    assert [[a.dtype for a in m] for m in got] == [[np.int64] * 2, [np.int64]] and got[1][0].tolist() == [5, 6, 7]
    for bad in (
        [[np.arange(4), np.arange(3)], [np.arange(3)]],  # a batch of another size
        [[np.arange(4)], [np.arange(3)]],  # a batch missing
        [[np.arange(4), np.arange(2)], [np.arange(3), np.arange(1)]],  # one too many
        [[np.arange(2), np.arange(4)], [np.arange(3)]],  # the sizes in another order
    ):
        with pytest.raises(ValueError, match="do not match"):
            _check_batches(sizes, bad)
    with pytest.raises(ValueError, match="2 members, 1 lists"):
        _check_batches(sizes, ok[:1])
    # graph ids outside the store never reach the descriptor gather
    for ids in ([5, 6, 8], [-1, 0, 1]):
        with pytest.raises(ValueError, match="outside the store"):
            _check_batches(sizes, [ok[0], [ids]], n_graphs=8)


def test_out_of_fold_argument_checks():
    models = [_g(), _g(), _g()]
    with pytest.raises(ValueError, match="one entry per member"):
        out_of_fold_predictions(models, None, [np.arange(3), np.arange(3, 6)])
    with pytest.raises(ValueError, match="held out more than once"):
        out_of_fold_predictions(models, None, [np.arange(4), np.arange(3, 6), np.arange(6, 9)])
    with pytest.raises(ValueError, match="held out more than once"):
        out_of_fold_predictions(models, None, [[0, 1, 1], [2], [3]])
    with pytest.raises(ValueError, match="GINet"):
        out_of_fold_predictions([_g(), FoutNet(30, 1)], None, [[0], [1]])


def test_ensemble_result_val_path_is_defaulted():
    r = EnsembleResult(np.zeros((1, 2)), None, [])
    assert r.val_path is None
