"""TEST INFRASTRUCTURE: the batch the tile route of GINet integrated gradients
is checked on beyond the graphs both fused routes take
(``test_gpu_integrated_gradients_tiles.py``, and on the CPU
``test_integrated_gradients_tiles_host.py``): three small graphs and one sized
from ``dr_ginet_integrated_grad_lds_bytes`` to exceed one workgroup's LDS in
the Z form (degree 8, of the order of N = 1 000), at position 2, with the
``ig_ref`` oracle's results on it (computed once, shared, unchanged).

Features are seeded normal draws (no two nodes alike: the pools have no ties,
``attribution_ref._synthetic``).  ``SEED`` is the data seed at which the fp32
oracle stays within a tenth of the tolerances of the fp64 reference for both
baselines (asserted by the host test): a disagreement on the GPU then cannot
be an arg-max that flips under fp32 rounding."""

from __future__ import annotations

import functools

import numpy as np
import torch

import ig_ref
from deeprank2_amd import _lib
from deeprank2_amd.utils.synthetic import make_dataset
from oracle import data_ref

LDS_MAX = 160 * 1024
F, OUT_DIM, TARGET, STEPS = 30, 2, 1, 8
LARGE_AT = 2  # the large graph's position
SEED = 81


@functools.lru_cache(maxsize=None)
def large_nodes():
    """The smallest N (a multiple of 100) whose Z-form integrated-gradient carve exceeds one workgroup's LDS by 8 KiB."""
    q = _lib.load().dr_ginet_integrated_grad_lds_bytes
    return next(n for n in range(600, 4000, 100) if q(n, 6 * n, F, 4, 12, 1, 1, OUT_DIM, 36) > LDS_MAX + 8 * 1024)


@functools.lru_cache(maxsize=None)
def datas(seed=SEED):
    n = large_nodes()
    (big,) = make_dataset(1, seed=seed, n_lo=n, n_hi=n, mean_degree=8.0, k_lo=4, k_hi=4)
    small = make_dataset(3, seed=seed + 1, n_lo=20, n_hi=60, mean_degree=6.0, k_lo=2, k_hi=13)
    graphs = [small[0], small[1], big, small[2]]
    rng = np.random.default_rng(seed)
    for g in graphs:
        g["x"] = rng.normal(size=g["x"].shape).astype(np.float32)
    return tuple(data_ref.synthetic_to_data(g, f"g{j}") for j, g in enumerate(graphs))


@functools.lru_cache(maxsize=None)
def baseline(kind, seed=SEED):
    """None (zeros) or the per-feature mean over the batch's nodes, fp32 ``[F]``."""
    if kind == "zero":
        return None
    assert kind == "mean"
    return torch.cat([d.x for d in datas(seed)]).mean(dim=0).to(torch.float32)


@functools.lru_cache(maxsize=None)
def reference(kind="zero", dtype=torch.float64, seed=SEED):
    """``ig_ref.integrated_gradients`` on the batch: target 1 of two outputs, 8 Gauss-Legendre nodes."""
    return ig_ref.integrated_gradients(ig_ref.oracle_model(F, OUT_DIM), datas(seed), TARGET, *ig_ref.nodes(STEPS), baseline(kind, seed), dtype)
