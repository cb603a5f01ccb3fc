"""TEST INFRASTRUCTURE shared by ``test_bf16_oracle.py`` (CPU) and
``test_gpu_bf16_parity.py`` (GPU): inputs with continuous features, one
training step of the bf16 oracle (``oracle/bf16_ref.py``), the tie guard on
the inputs, and the comparison both modules apply -- so the CPU sensitivity
test proves that the comparison the GPU test makes would notice a wrong
rounding point.
"""

from __future__ import annotations

import numpy as np
import pytest
import torch
from _util import assert_grad_close, fixed_dropout

from deeprank2_amd.utils.synthetic import make_dataset
from oracle import bf16_ref, data_ref
from oracle import pyg_ops as P

OUT_TOL = {"rtol": 1e-4, "atol": 1e-4}  # the project's fp32 tolerance (test_gpu_ginet.py, test_gpu_large.py)
LOSS_REL = 1e-4
GUARD = 1e-5  # about 100x the fp32 reorder noise of a <= 64-term dot product


def continuous_x(rng, n, f):
    """Seeded normals, each column scaled by a power of two drawn over four
    binades: no entry is exactly representable in bf16 (the synthetic
    generator's one-hot columns all are)."""
    return torch.from_numpy((rng.normal(size=(n, f)) * np.exp2(rng.uniform(-2.0, 2.0, size=f))).astype(np.float32))


def overwrite_x(datas, f, seed):
    rng = np.random.default_rng(seed)
    for d in datas:
        d.x = continuous_x(rng, d.x.shape[0], f)
    return datas


def make_inputs(n_graphs, f, seed, classes=0):
    """``n_graphs`` graphs of 60-200 nodes with 8-16 depth-0 clusters and
    continuous x of width ``f``; every second graph gets three depth-1
    clusters.  ``classes``: integer targets below it (cross entropy)."""
    datas = [data_ref.synthetic_to_data(g, f"c{i}") for i, g in enumerate(make_dataset(n_graphs, seed=seed, n_lo=60, n_hi=200, mean_degree=10.0, k_lo=8, k_hi=16))]
    for i, d in enumerate(datas):
        if i % 2:
            d.cluster1 = torch.tensor([j % 3 for j in range(len(d.cluster1))], dtype=torch.long)
        if classes:
            d.y = torch.tensor([float(i % classes)])
    return overwrite_x(datas, f, 7919 * seed + f)


def dropout_mask(b, seed=5):
    return (torch.rand(b, 128, generator=torch.Generator().manual_seed(seed)) >= 0.4).float()


def named_grads(model):
    return {n: (None if p.grad is None else p.grad.detach().numpy().copy()) for n, p in model.named_parameters()}


def oracle_step(model, datas, mask, loss="mse"):
    """Forward, loss and backward of ``model`` (an oracle GINet, already
    holding the parameters) on a fresh batch of ``datas`` with the fixed
    dropout ``mask``; returns the comparison record ``{"out", "loss", "grads"}``."""
    model.train()
    model.dropout_fn = fixed_dropout(mask)
    model.zero_grad()
    bat = P.Batch.from_data_list([d.clone() for d in datas])
    out = model(bat)
    lv = torch.nn.functional.mse_loss(out.reshape(-1), bat.y) if loss == "mse" else torch.nn.functional.cross_entropy(out, bat.y.long())
    lv.backward()
    return {"out": out.detach().numpy().copy(), "loss": float(lv.detach()), "grads": named_grads(model)}


def bf16_oracle(f, out_dim, seed, **quant):
    torch.manual_seed(seed)
    return bf16_ref.GINetBf16(f, out_dim, 3, **quant)


FEATURES = (1, 12, 20, 30, 33, 50, 64)  # XSB 8/16/24/32/40/56/64, KPB 32/64, nch 2..16, zero and non-zero Z pad columns
# data seed per case, chosen on the CPU so that the inputs pass the tie guard
# (test_bf16_oracle.py re-checks every one); the model seed is 100 + data seed
SEEDS = {1: 1, 12: 12, 20: 21, 30: 31, 33: 41, 50: 51, 64: 61, "ce": 71, "degenerate": 4}
_cache = {}


def case(key):
    """The inputs of one GPU parity case, built once per process and left
    unchanged: ``key`` in ``FEATURES`` (3 graphs, MSE), ``"ce"`` (4 graphs,
    F = 30, two classes, cross entropy) or ``"degenerate"``
    (``graph_zoo.degenerate()`` with continuous x on the synthetic graphs,
    less the graphs that alone fail the tie guard).  Returns a dict: ``datas``,
    ``f``, ``out_dim``, ``loss``, ``mask``, ``model`` (the bf16 oracle after
    its step: ``.trace``, parameters' ``.grad``), ``state`` (the parameters
    before the step), ``ref`` (the comparison record), ``dropped``."""
    if key in _cache:
        return _cache[key]
    seed = SEEDS[key]
    dropped = []
    if key == "degenerate":
        import graph_zoo  # noqa: PLC0415

        f, out_dim, loss = 30, 1, "mse"
        datas = graph_zoo.degenerate()
        overwrite_x(datas[5:], f, seed)  # the hand-made graphs' x is continuous already
        probe = bf16_oracle(f, out_dim, 100 + seed)
        oracle_step(probe, datas, dropout_mask(len(datas)), loss)
        dropped = sorted(tie_guard_failures(probe))
        assert len(dropped) <= 2, f"more than two graphs fail the tie guard ({dropped}): change the seed"  # noqa: PLR2004
        datas = [d for i, d in enumerate(datas) if i not in dropped]
    elif key == "ce":
        f, out_dim, loss = 30, 2, "ce"
        datas = make_inputs(4, f, seed, classes=2)
    else:
        f, out_dim, loss = int(key), 1, "mse"
        datas = make_inputs(3, f, seed)
    mask = dropout_mask(len(datas))
    model = bf16_oracle(f, out_dim, 100 + seed)
    state = {k: v.detach().clone() for k, v in model.state_dict().items()}
    ref = oracle_step(model, datas, mask, loss)
    _cache[key] = {"datas": datas, "f": f, "out_dim": out_dim, "loss": loss, "mask": mask, "model": model, "state": state, "ref": ref, "dropped": dropped}
    return _cache[key]


def _top2(src, index):
    """Per (segment, channel): the maximum and the largest value among the
    other members (-inf when the segment has one member)."""
    n = src.shape[0]
    size = int(index.max()) + 1
    best, arg = P.scatter_max(src, index, dim_size=size)
    rest = torch.cat([src, torch.full((1, src.shape[1]), -np.inf)])
    rest.scatter_(0, arg, -np.inf)  # arg = n for empty segments: the spare row
    second = torch.full((size, src.shape[1]), -np.inf)
    second.scatter_reduce_(0, index.view(-1, 1).expand(n, src.shape[1]), rest[:n], reduce="amax", include_self=True)
    return best, second


def tie_guard(model):
    """Graphs of the last forward of ``model`` (a ``GINetBf16``) on which an
    argmax could legitimately differ between two fp32 evaluation orders: for
    both conv branches, at the depth-0 and the depth-1 pool, a positive pooled
    maximum ``m`` whose runner-up exceeds ``m (1 - GUARD)`` or that is below
    ``GUARD * max|H|``.  Returns ({graph: [description, ...]}, number of
    positive maxima looked at); an empty dict passes.  A condition on the
    *inputs*: choose another seed, never relax it."""
    tr = model.trace
    bad = {}
    n_max = 0
    for level, hs, pools, batches in (("depth0", tr["h1"], tr["pool0"], tr["batch0"]), ("depth1", tr["h2"], tr["pool1"], tr["batch1"])):
        for branch, (h, (src, index), batch) in enumerate(zip(hs, pools, batches)):
            best, second = _top2(src, index)
            seg_graph = torch.zeros(best.shape[0], dtype=torch.long).scatter_(0, index, batch)
            pos = best > 0
            n_max += int(pos.sum())
            near = pos & (second > best * (1.0 - GUARD))
            tiny = pos & (best < GUARD * float(h.abs().max()))
            for what, m in (("runner-up within 1e-5", near), ("maximum below 1e-5 of max|H|", tiny)):
                for seg, ch in torch.nonzero(m).tolist():
                    bad.setdefault(int(seg_graph[seg]), []).append(f"{level} branch {branch} segment {seg} channel {ch}: {what} ({float(best[seg, ch])!r}, {float(second[seg, ch])!r})")
    return bad, n_max


def tie_guard_failures(model):
    return tie_guard(model)[0]


def assert_tie_guard(model):
    bad = tie_guard_failures(model)
    assert not bad, f"these inputs have near-tied or tiny pooled maxima (choose another seed): {bad}"


def normwise(a, r):
    a, r = np.asarray(a, np.float64), np.asarray(r, np.float64)
    return float(np.linalg.norm(a - r) / max(np.linalg.norm(r), 1e-30))


def measure(got, ref):
    """(largest |out - ref| / max|ref|, largest normwise gradient error) of two comparison records."""
    eo = float(np.abs(got["out"] - ref["out"]).max() / np.abs(ref["out"]).max())
    eg = max(normwise(got["grads"][n], g) for n, g in ref["grads"].items() if g is not None and np.any(g))
    return eo, eg


def assert_parity(got, ref, label=""):
    """THE comparison of the GPU parity tests, at the project's fp32
    tolerance: outputs rtol = atol = 1e-4, loss 1e-4 relative, every parameter
    gradient through ``assert_grad_close`` with its defaults, and exact zeros
    wherever the reference has no gradient (None) or an all-zero one (the
    attention parameters).  Prints the measured errors first."""
    eo, eg = measure(got, ref)
    print(f"[parity {label}] out err / max|out| = {eo:.3e}   worst normwise grad err = {eg:.3e}   loss {got['loss']!r} vs {ref['loss']!r}")
    np.testing.assert_allclose(got["out"], ref["out"], **OUT_TOL, err_msg=f"{label} out")
    assert got["loss"] == pytest.approx(ref["loss"], rel=LOSS_REL), label
    assert set(got["grads"]) == set(ref["grads"])
    for n, g in ref["grads"].items():
        a = got["grads"][n]
        if g is None or not np.any(g):
            assert a is None or not np.any(a), f"{label} {n}: expected exact zeros"
            continue
        assert a is not None, n
        assert_grad_close(a, g, err_msg=f"{label} {n}")
    return eo, eg
