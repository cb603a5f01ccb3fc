"""A numpy restatement of ``dr_ensemble_score`` (csrc/ensemble_score.hip): the
same row -> thread assignment (row i belongs to thread i % 256), the same
ascending walk per thread and the same tree over the 256 partials, in float64.

MSE and L1 form their fp32 term as the kernel does (one IEEE subtract, one
multiply or fabs), so for them every slot equals the kernel's bit for bit.
SmoothL1, Huber and the cross entropy start from the same fp32 values (and,
for the regression branches, take the comparison in fp32) but evaluate the
term in float64: slot 0 is then a reference at a tolerance, the other slots
stay exact.
"""

from __future__ import annotations

import numpy as np

NT = 256
SUMS = 12


def tree_sum(contrib):
    """[n, S] float64 row contributions -> [S]: thread t adds rows t, t + 256,
    ... in ascending order into zero, then v[t] += v[t + s] for s = 128 .. 1."""
    n, s = contrib.shape
    rounds = -(-n // NT) if n else 0
    padded = np.zeros((rounds * NT, s))
    padded[:n] = contrib
    v = np.zeros((NT, s))
    with np.errstate(all="ignore"):
        for r in range(rounds):
            v = v + padded[r * NT : (r + 1) * NT]  # (a row past n adds +0.0: no change)
        step = NT // 2
        while step:
            v[:step] = v[:step] + v[step : 2 * step]
            step //= 2
    return v[0]


def regress_terms(d, loss, param):
    """The per-row loss terms of residuals ``d`` (fp32) as float64; MSE and L1
    rounded to fp32 exactly as the kernel forms them."""
    d = d.astype(np.float32)
    ad = np.abs(d)
    with np.errstate(all="ignore"):
        if loss == "mse":
            return (d * d).astype(np.float64)
        if loss == "l1" or (loss == "smooth_l1" and param == 0.0):
            return ad.astype(np.float64)
        p32, p = np.float32(param), float(np.float32(param))
        dd, add = d.astype(np.float64), ad.astype(np.float64)
        small = ad < p32  # the branch is taken in fp32, as the kernel takes it
        if loss == "smooth_l1":
            t = np.where(small, 0.5 * dd * dd / p, add - 0.5 * p)
        elif loss == "huber":
            t = np.where(small, 0.5 * dd * dd, p * (add - 0.5 * p))
        else:
            raise ValueError(loss)
        return np.where(np.isnan(dd), np.nan, t)


def member_rows(out_k, y, ids, *, loss, param=0.0, class_w=None, probs=False):
    """One member's rows -> (contrib [n, 11] float64, confusion [C, C] int64 or
    None for a regression loss).  ``ids``: the graph id of every row."""
    n, c = out_k.shape
    ids = np.asarray(ids, dtype=np.int64)
    g_ok = (ids >= 0) & (ids < y.size)
    yv = np.where(g_ok, y[np.where(g_ok, ids, 0)], np.float32(0)).astype(np.float32)
    contrib = np.zeros((n, 11))
    with np.errstate(all="ignore"):
        if loss != "ce":
            o = out_k[:, 0].astype(np.float32)
            d = (o - yv).astype(np.float32)
            term = regress_terms(d, loss, param)
            dd, od, yd = d.astype(np.float64), o.astype(np.float64), yv.astype(np.float64)
            cols = [term, np.ones(n), np.isnan(term).astype(np.float64), np.zeros(n), dd * dd, np.abs(dd), od, yd, od * od, yd * yd, od * yd]
            contrib = np.stack(cols, axis=1)
            contrib[~g_ok] = 0.0
            contrib[~g_ok, 3] = 1.0
            return contrib, None
        y_ok = g_ok & (yv >= 0) & (yv < c) & (yv == np.floor(yv))
        yi = np.where(y_ok, yv, 0).astype(np.int64)
        o = out_k.astype(np.float64)
        nan = np.isnan(o).any(axis=1)
        oy = o[np.arange(n), yi]
        if probs:
            term = -np.log(oy)
        else:
            mx = np.fmax.reduce(o, axis=1)  # (skips NaN, as fmaxf does)
            term = mx + np.log(np.exp(o - mx[:, None]).sum(axis=1)) - oy
        w = np.ones(n) if class_w is None else class_w.astype(np.float32)[yi].astype(np.float64)
        best = np.zeros(n, dtype=np.int64)
        best_v = out_k[:, 0].copy()
        for q in range(1, c):  # strict: the lowest index among equals
            take = out_k[:, q] > best_v
            best, best_v = np.where(take, q, best), np.where(take, out_k[:, q], best_v)
        contrib[:, 0] = w * term
        contrib[:, 1] = w
        contrib[:, 2] = nan
        contrib[:, 4] = (~nan) & (best == yi)
        contrib[:, 5] = 1.0
        contrib[~y_ok] = 0.0
        contrib[~y_ok, 3] = 1.0
        conf = np.zeros((c, c), dtype=np.int64)
        use = y_ok & ~nan
        np.add.at(conf, (yi[use], best[use]), 1)
        return contrib, conf


def score_ref(out, y, n, *, gids=None, loss, param=0.0, class_w=None, probs=False):
    """``out`` [K, rows, C] fp32, ``y`` [G] fp32, ``n`` [K] row counts, ``gids``
    None (row i scores y[i]), [rows] (all members) or [K, rows] ->
    (sums [K, 12] float64, confusion [K, C, C] int64 or None)."""
    out = np.asarray(out, dtype=np.float32)
    y = np.asarray(y, dtype=np.float32)
    k = out.shape[0]
    sums = np.zeros((k, SUMS))
    confs = []
    for m in range(k):
        ids = np.arange(n[m]) if gids is None else np.asarray(gids)[: n[m]] if np.ndim(gids) == 1 else np.asarray(gids)[m, : n[m]]
        contrib, conf = member_rows(out[m, : n[m]], y, ids, loss=loss, param=param, class_w=class_w, probs=probs)
        sums[m, :11] = tree_sum(contrib)
        confs.append(conf)
    return sums, (None if loss != "ce" else np.stack(confs))
