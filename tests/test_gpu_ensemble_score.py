"""``dr_ensemble_score`` (``ensemble.ensemble_score``) against its numpy
restatement ``tests/score_ref.py`` on random predictions, targets and ids: no
model is needed.

MSE and L1: every slot equals the restatement bit for bit (the term is one IEEE
subtract and one multiply or fabs, the order of the adds is fixed).  SmoothL1,
Huber, cross entropy: slot 0 at the tolerances below, every other slot and the
confusion matrix exact.

* SmoothL1 / Huber: ``rtol = 1e-6``.  A non-negative term carries at most about
  five fp32 roundings, 5 * 2^-24 ~ 3e-7, which a sum of non-negative terms
  preserves.
* cross entropy: ``rtol = 1e-5`` plus ``1e-6 * max(1, max|logit|)`` per scored
  row: ``lse - o[y]`` cancels, expf / logf are good to a few ulp.
"""

from __future__ import annotations

import numpy as np
import pytest
import torch
from score_ref import score_ref

from deeprank2_amd.ensemble import ensemble_score, scores_from_sums

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G = 1000  # targets in the stand-in store
SIZES = (1, 255, 256, 257, 1000)


def _counts(k, n):
    """Unequal row counts, one of them 0 (K > 1), the first the full n."""
    return [n, 0, max(1, n // 2), n - 1, 1, n, n // 3, min(n, 7)][:k]


def _case(seed, k, n, out_dim, ids, classif, probs=False):
    """Random inputs: out [K, n, C] inside a wider buffer (members further than
    n * C apart), targets, and ids None / "rows" ([K, n]) / "shared" ([n])."""
    rng = np.random.default_rng(seed)
    buf = rng.normal(scale=3.0, size=(k, n + 3, out_dim)).astype(np.float32)
    if probs:
        e = np.exp(buf - buf.max(axis=2, keepdims=True))
        buf = (e / e.sum(axis=2, keepdims=True)).astype(np.float32)
    y = rng.integers(0, out_dim, size=G).astype(np.float32) if classif else rng.normal(size=G).astype(np.float32)
    gids = None if ids is None else rng.integers(0, G, size=(k, n + 5) if ids == "rows" else (n,)).astype(np.int64)
    return buf, y, gids


def _run(buf, y, gids, counts, n, **kw):
    out = torch.from_numpy(buf).to(DEV)[:, :n]
    t_gids = None if gids is None else torch.from_numpy(gids).to(DEV)
    sums, conf = ensemble_score(out, torch.from_numpy(y).to(DEV), gids=t_gids, n=counts, **kw)
    return sums.cpu().numpy(), None if conf is None else conf.cpu().numpy()


def _ref(buf, y, gids, counts, n, *, loss, loss_param=None, class_weights=None, probs=False, confusion=False):
    param = 0.0 if loss not in ("smooth_l1", "huber") else 1.0 if loss_param is None else loss_param
    return score_ref(buf[:, :n], y, counts, gids=gids, loss=loss, param=param, class_w=class_weights, probs=probs)


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize("k", [1, 3, 8])
@pytest.mark.parametrize("loss", ["mse", "l1", "smooth_l1_beta0"])
def test_mse_and_l1_sums_equal_the_restatement_bit_for_bit(loss, k):
    kw = dict(loss="smooth_l1", loss_param=0.0) if loss == "smooth_l1_beta0" else dict(loss=loss)  # (beta 0 is L1)
    for n in SIZES:
        for out_dim in (1, 3):
            for ids in (None, "rows", "shared"):
                buf, y, gids = _case(1000 * k + n + out_dim, k, n, out_dim, ids, False)
                counts = _counts(k, n)
                got, conf = _run(buf, y, gids, counts, n, **kw)
                want, _ = _ref(buf, y, gids, counts, n, **kw)
                assert conf is None
                assert _same(got, want), (n, out_dim, ids, np.abs(got - want).max())
                assert (got[:, 1] == counts).all() and (got[:, 11] == 0).all()


@pytest.mark.parametrize("k", [1, 3, 8])
@pytest.mark.parametrize("loss,param", [("smooth_l1", None), ("smooth_l1", 0.3), ("huber", None), ("huber", 2.5)])
def test_smooth_l1_and_huber_within_rtol(loss, param, k):
    worst = 0.0
    for n in SIZES:
        for ids in (None, "rows", "shared"):
            buf, y, gids = _case(77 * k + n, k, n, 2, ids, False)
            counts = _counts(k, n)
            got, _ = _run(buf, y, gids, counts, n, loss=loss, loss_param=param)
            want, _ = _ref(buf, y, gids, counts, n, loss=loss, loss_param=param)
            assert _same(got[:, 1:], want[:, 1:]), (n, ids)  # every other slot is exact
            err = np.abs(got[:, 0] - want[:, 0]) / np.maximum(np.abs(want[:, 0]), 1e-300)
            worst = max(worst, float(np.where(want[:, 0] == 0, got[:, 0] != 0, err).max()))
    print(f"{loss}({param}) K={k}: worst relative error of slot 0 = {worst:.3e}")
    assert worst <= 1e-6  # noqa: PLR2004


@pytest.mark.parametrize("k", [1, 3, 8])
@pytest.mark.parametrize("out_dim", [2, 3, 16])
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("probs", [False, True], ids=["logits", "probs"])
def test_cross_entropy_within_tolerance_and_counts_exact(probs, weighted, out_dim, k):
    cw = np.random.default_rng(out_dim).uniform(0.5, 2.0, size=out_dim).astype(np.float32) if weighted else None
    worst = 0.0
    for n in SIZES:
        for ids in (None, "rows", "shared"):
            buf, y, gids = _case(31 * k + n + out_dim, k, n, out_dim, ids, True, probs)
            counts = _counts(k, n)
            kw = dict(loss="ce", class_weights=cw, probs=probs, confusion=True)
            got, conf = _run(buf, y, gids, counts, n, **kw)
            want, wconf = _ref(buf, y, gids, counts, n, **kw)
            assert _same(got[:, 1:], want[:, 1:]), (n, ids)  # sum of weights, counts, correct rows: exact
            assert np.array_equal(conf, wconf) and conf.sum(axis=(1, 2)).tolist() == counts
            tol = 1e-5 * np.abs(want[:, 0]) + 1e-6 * max(1.0, float(np.abs(buf).max())) * np.asarray(counts)
            err = np.abs(got[:, 0] - want[:, 0])
            assert (err <= tol).all(), (n, ids, err, tol)
            worst = max(worst, float((err / np.maximum(tol, 1e-300)).max()))
            acc = scores_from_sums(got, conf, "classif").accuracy
            assert _same(acc, np.where(np.asarray(counts) > 0, np.trace(conf, axis1=1, axis2=2) / np.maximum(counts, 1), np.nan))
    print(f"ce C={out_dim} K={k} probs={probs} weighted={weighted}: worst error / tolerance = {worst:.3e}")


def test_ties_take_the_lowest_label():
    out = torch.tensor([[[1.0, 1.0, 0.0], [0.0, 2.0, 2.0], [3.0, 3.0, 3.0]]], device=DEV)
    y = torch.tensor([1.0, 1.0, 0.0], device=DEV)
    sums, conf = ensemble_score(out, y, loss="ce", confusion=True)
    assert conf[0].tolist() == [[1, 0, 0], [1, 1, 0], [0, 0, 0]] and sums[0, 4].item() == 2.0  # noqa: PLR2004


@pytest.mark.parametrize("classif", [False, True], ids=["regress", "classif"])
def test_rows_with_bad_ids_or_targets_are_counted_and_left_out(classif):
    """Ids of -1 and G, and for a classifier targets of -1, out_dim, 0.5 and
    NaN: slot 3 counts exactly those rows and every other slot equals the
    score of the remaining rows.  Such a value is only compared in the kernel,
    never used as an index."""
    k, n, c = 3, 300, 3
    rng = np.random.default_rng(5)
    buf = rng.normal(size=(k, n, c)).astype(np.float32)
    y = (rng.integers(0, c, size=G) if classif else rng.normal(size=G)).astype(np.float32)
    gids = rng.integers(0, G - 8, size=(k, n)).astype(np.int64)
    bad = np.zeros((k, n), dtype=bool)
    for m in range(k):
        rows = rng.choice(n, size=12, replace=False)
        gids[m, rows[:3]], gids[m, rows[3:6]] = -1, G
        bad[m, rows[:6]] = True
        if classif:  # the last 8 targets are no class index; the clean ids never point there
            y[G - 8 :] = [-1.0, c, 0.5, np.nan, -0.5, c + 0.5, np.inf, -np.inf]
            gids[m, rows[6:12]] = G - 8 + np.arange(6) + (m % 3)
            bad[m, rows[6:12]] = True
    kw = dict(loss="ce", confusion=True) if classif else dict(loss="mse")
    got, conf = _run(buf, y, gids, [n] * k, n, **kw)
    assert got[:, 3].tolist() == bad.sum(axis=1).tolist()
    for m in range(k):
        keep = ~bad[m]
        want, wconf = score_ref(buf[m : m + 1, keep], y, [int(keep.sum())], gids=gids[m, keep], loss=kw["loss"])
        if classif:
            assert np.array_equal(conf[m], wconf[0])
            assert _same(got[m, [1, 2, 4, 5]], want[0, [1, 2, 4, 5]])
        else:
            # the same rows in another thread assignment: the sums agree to rounding, the counts exactly
            assert got[m, 1] == want[0, 1] and got[m, 2] == 0
            np.testing.assert_allclose(got[m, [0, 4, 5, 6, 7, 8, 9, 10]], want[0, [0, 4, 5, 6, 7, 8, 9, 10]], rtol=1e-12, atol=1e-12)
    # and with the rows in place, the restatement leaves them out the same way: bit for bit
    want, wconf = score_ref(buf, y, [n] * k, gids=gids, loss=kw["loss"])
    if classif:
        assert _same(got[:, 1:], want[:, 1:]) and np.array_equal(conf, wconf)
        np.testing.assert_allclose(got[:, 0], want[:, 0], rtol=1e-5, atol=1e-6 * n * max(1.0, float(np.abs(buf).max())))
    else:
        assert _same(got, want)


@pytest.mark.parametrize("loss", ["mse", "huber", "ce"])
def test_a_nan_prediction_turns_only_its_members_loss_nan(loss):
    k, n, c = 3, 257, 2
    buf, y, gids = _case(9, k, n, c, "rows", loss == "ce")
    counts = [n, n - 1, 100]
    kw = dict(loss=loss, confusion=True) if loss == "ce" else dict(loss=loss)
    clean, cconf = _run(buf, y, gids, counts, n, **kw)
    dirty = buf.copy()
    dirty[1, 40, 0] = np.nan
    dirty[1, 41, 1] = np.nan  # (column 1: read by the classifier only)
    got, conf = _run(dirty, y, gids, counts, n, **kw)
    assert _same(got[[0, 2]], clean[[0, 2]])
    assert np.isnan(got[1, 0]) and got[1, 2] == (2 if loss == "ce" else 1) and got[1, 1] == clean[1, 1] and got[1, 3] == 0
    s = scores_from_sums(got, conf, "classif" if loss == "ce" else "regress")
    assert np.isnan(s.loss[1]) and np.isfinite(s.loss[[0, 2]]).all()
    if loss == "ce":
        assert np.array_equal(conf[[0, 2]], cconf[[0, 2]]) and conf[1].sum() == counts[1] - 2 and got[1, 5] == counts[1]
        want, wconf = _ref(dirty, y, gids, counts, n, **kw)
        assert np.array_equal(conf, wconf) and _same(got[:, 1:], want[:, 1:])


def test_two_launches_give_the_same_bits():
    k, n, c = 8, 1000, 16
    buf, y, gids = _case(3, k, n, c, "rows", True)
    out, ty, tg = torch.from_numpy(buf).to(DEV)[:, :n], torch.from_numpy(y).to(DEV), torch.from_numpy(gids).to(DEV)
    for kw in (dict(loss="ce", confusion=True), dict(loss="huber", loss_param=0.7), dict(loss="mse")):
        a, ca = ensemble_score(out, ty, gids=tg, n=_counts(k, n), **kw)
        b, cb = ensemble_score(out, ty, gids=tg, n=_counts(k, n), **kw)
        assert torch.equal(a, b) and (ca is None or torch.equal(ca, cb))
        assert a.shape == (k, 12) and a.dtype == torch.float64 and (ca is None or (ca.shape == (k, c, c) and ca.dtype == torch.int64))


def test_wrapper_refusals():
    out, y = torch.zeros(2, 4, 2, device=DEV), torch.zeros(8, device=DEV)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ensemble_score(out.cpu(), y, loss="mse")
    for kw in (dict(loss="nll"), dict(loss="mse", probs=True), dict(loss="mse", confusion=True), dict(loss="mse", n=[5, 1]), dict(loss="mse", n=[1]), dict(loss="mse", gids=torch.zeros(3, dtype=torch.int64, device=DEV)),
               dict(loss="mse", gids=torch.zeros(4, dtype=torch.int32, device=DEV)), dict(loss="ce", class_weights=[1.0, 2.0, 3.0])):  # fmt: skip
        with pytest.raises(ValueError):
            ensemble_score(out, y, **kw)
    with pytest.raises(ValueError, match="more rows than targets"):
        ensemble_score(torch.zeros(1, 9, 1, device=DEV), y, loss="mse")
