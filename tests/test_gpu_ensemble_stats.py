"""``dr_ensemble_stats`` on synthetic member outputs (no model): the ensemble's
mean and spread as ``include/deeprank2_amd.h`` states their arithmetic.

* Regression mean: bit for bit a numpy float32 restatement of the chain
  ``s = o_0; s += o_k; s / K`` (IEEE adds and one IEEE divide).
* Regression spread, classification probabilities and entropy: against float64
  numpy at the project's output tolerance (rtol = atol = 1e-4).  The
  two-pass deviation of o ~ N(mu, 1), |mu| <= 10, carries an absolute error of
  about |mean| 2^-24 K <= 1e-5, so the tolerance holds for every element.
* Labels: on logits with one class per graph raised by 3 in every member, which
  separates the reference's top two mean probabilities by more than 1e-3
  (asserted on the reference), so every label must match.
"""

from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

from deeprank2_amd import _lib
from deeprank2_amd.ensemble import ensemble_stats

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = dict(rtol=1e-4, atol=1e-4)
NS = [1, 63, 64, 65, 255, 256, 257]  # one below, at and above the wave (64) and the block (256)
KS = [1, 2, 3, 8]
DIMS = [1, 2, 3, 16]
SENTINEL = -777.0


@functools.lru_cache(maxsize=None)
def _inputs(n, k, out_dim, kind):
    """Member outputs [k, n, out_dim] (float32, host) and, for the labels, the raised class per graph."""
    rng = np.random.default_rng(1000 * n + 10 * k + out_dim)
    if kind == "regress":
        mu = rng.uniform(-10.0, 10.0, size=(1, n, out_dim))
        o = (mu + rng.normal(size=(k, n, out_dim))).astype(np.float32)
        o.setflags(write=False)
        return o, None
    # logits N(0, 0.3^2) with one class per graph raised by 3 in every member: the raised
    # class leads every other by 3 + N(0, 0.18), seven standard deviations above zero
    top = rng.integers(0, out_dim, size=n)
    o = 0.3 * rng.normal(size=(k, n, out_dim))
    o[:, np.arange(n), top] += 3.0
    o = o.astype(np.float32)
    o.setflags(write=False)
    return o, top


def _run(o, kind, stride_pad=0):
    """dr_ensemble_stats on host array ``o`` through buffers one row longer
    than n, pre-filled with a sentinel: (mean, spread, label) with that row."""
    k, n, c = o.shape
    buf = torch.full((k, n * c + stride_pad), 12345.0, dtype=torch.float32, device=DEV)
    buf[:, : n * c] = torch.from_numpy(np.array(o)).to(DEV).reshape(k, n * c)
    classif = kind == "classif"
    mean = torch.full((n + 1, c), SENTINEL, dtype=torch.float32, device=DEV)
    spread = torch.full((n + 1,) if classif else (n + 1, c), SENTINEL, dtype=torch.float32, device=DEV)
    label = torch.full((n + 1,), -777, dtype=torch.int32, device=DEV)
    rc = _lib.load().dr_ensemble_stats(buf.data_ptr(), buf.stride(0), k, n, c, _lib.DR_ENS_CLASSIF if classif else _lib.DR_ENS_REGRESS,
                                       mean.data_ptr(), spread.data_ptr(), label.data_ptr() if classif else None, _lib.stream_ptr(torch.device(DEV)))  # fmt: skip
    assert rc == 0
    torch.cuda.synchronize()
    # rows past n keep the sentinel
    assert bool((mean[n] == SENTINEL).all()) and bool((spread[n] == SENTINEL).all()) and int(label[n]) == -777  # noqa: PLR2004
    if not classif:
        assert bool((label == -777).all()), "regression does not touch label"  # noqa: PLR2004
    return mean[:n].cpu().numpy(), spread[:n].cpu().numpy(), label[:n].cpu().numpy()


def _mean_chain_f32(o):
    s = o[0].astype(np.float32).copy()
    for k in range(1, o.shape[0]):
        s = (s + o[k]).astype(np.float32)
    return (s / np.float32(o.shape[0])).astype(np.float32)


def _softmax64(o):
    e = np.exp(o.astype(np.float64) - o.astype(np.float64).max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


@pytest.mark.parametrize("out_dim", DIMS)
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("n", NS)
def test_regression_mean_bit_for_bit_and_spread(n, k, out_dim):
    o, _ = _inputs(n, k, out_dim, "regress")
    mean, spread, _ = _run(o, "regress", stride_pad=5 if (n, k) == (65, 3) else 0)
    assert np.array_equal(mean.view(np.int32), _mean_chain_f32(o).view(np.int32))
    if k == 1:
        assert np.isnan(spread).all(), "one member: NaN, as torch.std"
    else:
        np.testing.assert_allclose(spread, o.astype(np.float64).std(axis=0, ddof=1), **TOL)


@pytest.mark.parametrize("out_dim", DIMS)
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("n", NS)
def test_classification_mean_entropy_and_labels(n, k, out_dim):
    o, top = _inputs(n, k, out_dim, "classif")
    mean, entropy, label = _run(o, "classif", stride_pad=3 if (n, k) == (257, 8) else 0)
    ref = _softmax64(o).mean(axis=0)
    np.testing.assert_allclose(mean, ref, **TOL)
    np.testing.assert_allclose(entropy, -(ref * np.log(ref)).sum(axis=-1), **TOL)
    if out_dim > 1:
        srt = np.sort(ref, axis=-1)
        assert (srt[:, -1] - srt[:, -2] > 1e-3).all(), "the reference's top two classes are separated"  # noqa: PLR2004
        assert np.array_equal(ref.argmax(axis=-1), top)
    assert np.array_equal(label, ref.argmax(axis=-1).astype(np.int32))


def test_stats_match_torch_on_the_wrapper():
    """``ensemble.ensemble_stats`` (what ``predict_ensemble`` calls), on a
    strided view: torch's own mean / std / softmax within the tolerance."""
    o, _ = _inputs(257, 3, 3, "regress")
    big = torch.zeros(3, 300, 3, device=DEV)
    big[:, :257] = torch.from_numpy(np.array(o)).to(DEV)
    view = big[:, :257]
    mean, spread, label = ensemble_stats(view, "regress")
    assert label is None and mean.shape == (257, 3) and spread.shape == (257, 3)
    torch.testing.assert_close(mean, view.mean(0), **TOL)
    torch.testing.assert_close(spread, view.std(0), **TOL)
    mean, entropy, label = ensemble_stats(view, "classif")
    p = torch.softmax(view, -1).mean(0)
    torch.testing.assert_close(mean, p, **TOL)
    torch.testing.assert_close(entropy, -(p * p.log()).sum(-1), **TOL)
    assert label.dtype == torch.int32 and entropy.shape == (257,)
    with pytest.raises(ValueError, match="task"):
        ensemble_stats(view, "rank")
    with pytest.raises(ValueError, match="contiguous"):
        ensemble_stats(big[:, ::2], "regress")


@pytest.mark.parametrize("out_dim", [1, 2, 3, 16])
def test_exact_tie_gives_label_zero_and_full_entropy(out_dim):
    o = np.zeros((3, 65, out_dim), np.float32)
    mean, entropy, label = _run(o, "classif")
    assert (label == 0).all()
    np.testing.assert_allclose(entropy, np.full(65, np.log(out_dim)), **TOL)
    np.testing.assert_allclose(mean, np.full((65, out_dim), 1.0 / out_dim), **TOL)


def test_nan_stays_with_its_graph():
    n, k, c = 130, 3, 3
    o, _ = _inputs(n, k, c, "classif")
    o = o.copy()
    o[1, 64, 2] = np.nan  # one logit of one member of graph 64
    clean, _ = _inputs(n, k, c, "classif")
    mean, entropy, label = _run(o, "classif")
    mean0, entropy0, label0 = _run(clean, "classif")
    assert np.isnan(mean[64]).all() and np.isnan(entropy[64]) and label[64] == -1
    rest = np.arange(n) != 64  # noqa: PLR2004
    assert np.array_equal(mean[rest], mean0[rest]) and np.array_equal(entropy[rest], entropy0[rest]) and np.array_equal(label[rest], label0[rest])
    assert (label[rest] >= 0).all()
    # regression: the NaN reaches the mean and the spread of that element only
    r, _ = _inputs(n, k, c, "regress")
    r = r.copy()
    r[2, 7, 1] = np.nan
    mean, spread, _ = _run(r, "regress")
    bad = np.zeros((n, c), bool)
    bad[7, 1] = True
    assert np.array_equal(np.isnan(mean), bad) and np.array_equal(np.isnan(spread), bad)
