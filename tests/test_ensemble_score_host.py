"""The host side of the device-formed validation scores: the refusals of
``dr_ensemble_score`` (made before any HIP call, so they need no device),
``scores_from_sums`` against hand-computed sums, the early-stopping
bookkeeping of ``train_ensemble`` on scripted losses, and the restatement
``tests/score_ref.py`` on a case small enough to add up by hand.
"""

from __future__ import annotations

import ctypes
import math

import numpy as np
import pytest
from score_ref import score_ref, tree_sum

from deeprank2_amd import _lib
from deeprank2_amd.ensemble import MemberStopping, ScoreSpec, scores_from_sums, train_ensemble

E_ARG = -1
MSE, CE, L1, SMOOTH, HUBER = _lib.DR_LOSS_MSE, _lib.DR_LOSS_CE, _lib.DR_LOSS_L1, _lib.DR_LOSS_SMOOTH_L1, _lib.DR_LOSS_HUBER


def _call(**kw):
    """dr_ensemble_score on small host buffers standing in for device memory: a
    refused call never reads them (and never reaches HIP)."""
    lib = _lib.load()
    buf = np.zeros(4096, dtype=np.float64)
    p = buf.ctypes.data
    a = dict(out=p, member_stride=64, gids=None, gid_stride=0, y=p, n_graphs=8, n=[4, 4], n_members=None, out_dim=1, loss_kind=MSE, loss_param=0.0, class_w=None, flags=0, sums=p, confusion=None)
    a.update(kw)
    n = (ctypes.c_int32 * _lib.DR_MAX_MEMBERS)(*a["n"])
    k = len(a["n"]) if a["n_members"] is None else a["n_members"]
    return lib.dr_ensemble_score(a["out"], a["member_stride"], a["gids"], a["gid_stride"], a["y"], a["n_graphs"], n, k, a["out_dim"], a["loss_kind"], a["loss_param"], a["class_w"], a["flags"], a["sums"], a["confusion"], None)


REFUSED = {
    "null out": dict(out=None),
    "null y": dict(y=None),
    "null sums": dict(sums=None),
    "no member": dict(n=[], n_members=0),
    "nine members": dict(n=[1] * 8, n_members=9),
    "out_dim 0": dict(out_dim=0),
    "out_dim 17": dict(out_dim=17, member_stride=1024),
    "negative n": dict(n=[4, -1]),
    "members overlap": dict(n=[4, 65], member_stride=64),
    "members overlap (out_dim)": dict(n=[4, 4], out_dim=3, loss_kind=CE, member_stride=11),
    "no loss": dict(loss_kind=_lib.DR_LOSS_NONE),
    "unknown loss": dict(loss_kind=6),
    "negative loss kind": dict(loss_kind=-1),
    "smooth_l1 beta < 0": dict(loss_kind=SMOOTH, loss_param=-1.0),
    "smooth_l1 beta nan": dict(loss_kind=SMOOTH, loss_param=math.nan),
    "huber delta 0": dict(loss_kind=HUBER, loss_param=0.0),
    "huber delta inf": dict(loss_kind=HUBER, loss_param=math.inf),
    "ce with one output": dict(loss_kind=CE, out_dim=1),
    "probs with a regression loss": dict(flags=_lib.DR_SCORE_PROBS),
    "probs with l1": dict(loss_kind=L1, flags=_lib.DR_SCORE_PROBS),
    "confusion with a regression loss": dict(confusion=1),
    "unknown flag": dict(loss_kind=CE, out_dim=2, flags=2),
    "negative store size": dict(n_graphs=-1),
    "negative gid stride": dict(gid_stride=-4),
}


@pytest.mark.parametrize("case", sorted(REFUSED))
def test_refusals_are_made_on_the_host(case):
    kw = dict(REFUSED[case])
    if kw.get("confusion") == 1:
        kw["confusion"] = np.zeros(64, dtype=np.int64).ctypes.data
    assert _call(**kw) == E_ARG


def test_constants_match_the_header():
    assert _lib.DR_SCORE_SUMS == 12 and _lib.DR_SCORE_PROBS == 1  # noqa: PLR2004


def test_score_spec_refuses_what_the_entry_refuses():
    assert ScoreSpec("huber").checked(1).loss_param == 1.0
    assert ScoreSpec("mse", 3.0).checked(1).loss_param == 0.0
    for spec, out_dim in ((ScoreSpec("nll"), 1), (ScoreSpec("huber", 0.0), 1), (ScoreSpec("smooth_l1", -1.0), 1), (ScoreSpec("ce"), 1), (ScoreSpec("mse", confusion=True), 1)):
        with pytest.raises(ValueError):
            spec.checked(out_dim)


# ---- scores_from_sums ----
def test_regression_scores_by_hand():
    # o = [1, 2, 4], y = [1, 3, 2]: d = [0, -1, 2]
    o, y = np.array([1.0, 2.0, 4.0]), np.array([1.0, 3.0, 2.0])
    d = o - y
    s = np.zeros((3, 12))
    s[0, :11] = [5.0, 3, 0, 2, (d * d).sum(), np.abs(d).sum(), o.sum(), y.sum(), (o * o).sum(), (y * y).sum(), (o * y).sum()]
    s[1, :11] = [0, 0, 0, 7, 0, 0, 0, 0, 0, 0, 0]  # every row left out
    s[2, :11] = [2.0, 2, 0, 0, 2.0, 2.0, 4.0, 6.0, 8.0, 18.0, 12.0]  # o = [2, 2], y = [3, 3]: no variance
    r = scores_from_sums(s, None, "regress")
    assert r.n.tolist() == [3, 0, 2] and r.n_skipped.tolist() == [2, 7, 0] and r.n_nan.tolist() == [0, 0, 0]
    assert r.loss[0] == 5.0 / 3 and r.rmse[0] == math.sqrt(5.0 / 3) and r.mae[0] == 1.0
    assert r.pearson[0] == pytest.approx(np.corrcoef(o, y)[0, 1], rel=1e-14)
    assert r.r2[0] == pytest.approx(1.0 - 5.0 / ((y - y.mean()) ** 2).sum(), rel=1e-14)
    for f in (r.loss, r.rmse, r.mae, r.pearson, r.r2):
        assert math.isnan(f[1])
    assert r.loss[2] == 1.0 and r.rmse[2] == 1.0 and math.isnan(r.pearson[2]) and math.isnan(r.r2[2])
    assert r.accuracy is None and r.confusion is None and r.mcc is None
    with pytest.raises(ValueError):
        scores_from_sums(s, np.zeros((3, 2, 2)), "regress")
    with pytest.raises(ValueError):
        scores_from_sums(s, None, "ranking")


def test_nan_sums_read_nan():
    s = np.zeros((1, 12))
    s[0, :11] = [math.nan, 4, 1, 0, math.nan, math.nan, math.nan, 4.0, math.nan, 6.0, math.nan]
    r = scores_from_sums(s, None, "regress")
    assert math.isnan(r.loss[0]) and math.isnan(r.rmse[0]) and r.n_nan[0] == 1 and r.n[0] == 4  # noqa: PLR2004


def test_classification_scores_by_hand():
    s = np.zeros((3, 12))
    conf = np.zeros((3, 2, 2), dtype=np.int64)
    s[0, :6] = [6.0, 12.0, 1, 2, 7, 11]  # 11 rows scored, one of them NaN
    conf[0] = [[4, 2], [1, 3]]  # tn fp / fn tp
    s[1, :6] = [0, 0, 0, 5, 0, 0]
    s[2, :6] = [1.5, 3.0, 0, 0, 3, 3]
    conf[2] = [[3, 0], [0, 0]]  # one class only
    r = scores_from_sums(s, conf, "classif")
    assert r.loss[0] == 0.5 and r.accuracy[0] == 7 / 11 and r.n.tolist() == [11, 0, 3] and r.n_nan.tolist() == [1, 0, 0]
    assert r.tpr[0] == 3 / 4 and r.tnr[0] == 4 / 6 and r.precision[0] == 3 / 5
    assert r.mcc[0] == pytest.approx((3 * 4 - 2 * 1) / math.sqrt(5 * 4 * 6 * 5), rel=1e-15)
    assert np.array_equal(r.confusion, conf)
    for f in (r.loss, r.accuracy, r.tpr, r.tnr, r.precision, r.mcc):
        assert math.isnan(f[1])
    assert r.accuracy[2] == 1.0 and r.tnr[2] == 1.0 and math.isnan(r.tpr[2]) and math.isnan(r.precision[2]) and math.isnan(r.mcc[2])
    assert r.rmse is None and r.pearson is None
    r3 = scores_from_sums(s, np.zeros((3, 3, 3), dtype=np.int64), "classif")
    assert r3.confusion.shape == (3, 3, 3) and r3.mcc is None and r3.tpr is None
    assert scores_from_sums(s, None, "classif").confusion is None


# ---- the early-stopping bookkeeping ----
def _script(patience, min_delta, rows):
    st = MemberStopping(len(rows[0]), patience, min_delta)
    active = []
    for e, row in enumerate(rows):
        active.append(st.active.tolist())
        st.update(e, row)
    return st, active


def test_stopping_counts_an_improvement_below_min_delta_as_none():
    st, active = _script(2, 0.1, [[1.0, 1.0], [0.95, 0.8], [0.91, 0.75], [0.5, 0.74]])
    # member 0: 0.95 and 0.91 are within 0.1 of its best 1.0 -> stopped after epoch 2, best stays epoch 0;
    # member 1: improves at 1; 0.75 and 0.74 do not beat 0.8 - 0.1 -> stopped after epoch 3
    assert st.stopped_epoch.tolist() == [2, 3] and st.best_epoch.tolist() == [0, 1] and st.best.tolist() == [1.0, 0.8]
    assert active == [[True, True], [True, True], [True, True], [False, True]]


def test_stopping_takes_nan_as_no_improvement():
    st, _ = _script(2, 0.0, [[math.nan, 1.0], [math.nan, math.nan], [0.5, 0.9]])
    assert st.stopped_epoch.tolist() == [1, -1] and st.best_epoch.tolist() == [-1, 2]
    st, _ = _script(2, 0.0, [[1.0], [math.nan], [math.nan]])
    assert st.stopped_epoch.tolist() == [2] and st.best_epoch.tolist() == [0]


def test_stopping_with_patience_one_and_equal_losses():
    st, active = _script(1, 0.0, [[1.0, 1.0], [1.0, 0.9], [0.1, 0.8]])
    assert st.stopped_epoch.tolist() == [1, -1] and st.best_epoch.tolist() == [0, 2]  # an equal loss is no improvement
    assert active[2] == [False, True]
    assert st.update(3, [0.0, 0.7]) == [1]  # a stopped member's entry is ignored


def test_never_stopping():
    st, _ = _script(None, 0.0, [[3.0], [4.0], [5.0], [2.0], [6.0]])
    assert st.stopped_epoch.tolist() == [-1] and st.best_epoch.tolist() == [3] and bool(st.active.all())
    st, _ = _script(3, 0.0, [[3.0], [4.0], [5.0], [2.0], [6.0], [7.0]])
    assert st.stopped_epoch.tolist() == [-1] and st.best_epoch.tolist() == [3]
    for bad in (dict(patience=0), dict(min_delta=-1.0), dict(min_delta=math.nan)):
        with pytest.raises(ValueError):
            MemberStopping(2, **bad)


@pytest.mark.parametrize("kw", [dict(patience=2), dict(restore_best=True), dict(val_loss="device")], ids=lambda kw: next(iter(kw)))
def test_stopping_needs_held_out_graphs(kw):
    with pytest.raises(ValueError, match="val_indices"):
        train_ensemble([], None, **kw)
    with pytest.raises(ValueError, match="val_loss"):
        train_ensemble([], None, val_loss="both")


# ---- the restatement itself ----
def test_score_ref_adds_up_a_small_case_by_hand():
    out = np.array([[[1.0], [2.0], [4.0], [9.0]]], dtype=np.float32)
    y = np.array([1.0, 3.0, 2.0], dtype=np.float32)
    sums, conf = score_ref(out, y, [4], gids=np.array([0, 1, 2, 3]), loss="mse")
    assert conf is None and sums[0].tolist() == [5.0, 3.0, 0.0, 1.0, 5.0, 3.0, 7.0, 6.0, 21.0, 14.0, 15.0, 0.0]
    logits = np.array([[[0.0, 0.0], [2.0, 1.0], [0.0, 3.0], [1.0, 1.0]]], dtype=np.float32)
    sums, conf = score_ref(logits, np.array([0.0, 1.0, 1.0, 0.5], dtype=np.float32), [4], loss="ce")
    want = math.log(2.0) + (2.0 + math.log(1.0 + math.exp(-1.0)) - 1.0) + (3.0 + math.log(1.0 + math.exp(-3.0)) - 3.0)
    assert sums[0, 0] == pytest.approx(want, rel=1e-15) and sums[0, 1:6].tolist() == [3.0, 0.0, 1.0, 2.0, 3.0]
    assert conf[0].tolist() == [[1, 0], [1, 1]]  # equal logits: label 0


def test_tree_sum_order():
    # thread 0 adds rows 0 and 256 first, then the tree: (1e16 + 1) + (-1e16) in that order loses the 1
    c = np.zeros((257, 1))
    c[0], c[256], c[128] = 1e16, 1.0, -1e16
    assert tree_sum(c)[0] == 0.0
    c[0], c[256], c[128] = 1e16, -1e16, 1.0
    assert tree_sum(c)[0] == 1.0
