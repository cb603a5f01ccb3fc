"""The cases of ``width_cases.py`` are what they claim (host only): the layout
values the FoutNet / SGAT kernels derive from F, OUT and K0 take every value
``test_gpu_widths.py`` is meant to reach, every batch keeps its transposed
arrays apart, the fp64 oracle is finite with non-zero gradients, and the fp32
oracle stays within a tenth of the GPU comparison's tolerance of the fp64 one,
so that comparison's budget is the kernel's.

Largest fp32-oracle ratio per family, as this module measures it (``pytest
-s`` prints every case): FoutNet 0.011, SGAT 0.036 (edge weights / 6),
ginet_nocluster 0.082, GINet 0.040, k0_over_64 0.020.
"""

from __future__ import annotations

import ctypes

import numpy as np
import pytest
import torch
import width_cases as W

import graph_zoo
from deeprank2_amd import _lib

LDS_MAX = 160 * 1024
HEADROOM = 0.1  # of the GPU comparison's tolerance: a condition on the inputs, not a measurement
FOUT_CASES = [c for c in W.all_cases() if c[0] in ("foutnet", "sgat")]
IDS = lambda c: f"{c[0]}-F{c[1]}-OUT{c[2]}-{c[3]}"  # noqa: E731


def _carve(kind, q):
    arr = (ctypes.c_int32 * len(q))(*q)
    buf = ctypes.create_string_buffer(8192)
    n = getattr(_lib.load(), f"dr_debug_carve_{kind}")(arr, buf, 8192)
    assert 0 < n < 8192  # noqa: PLR2004
    return {k: int(v) for k, v in (part.split("=") for part in buf.value.decode().split(";") if part)}


def _layout(family, f, out, batch):
    """What fout_graph_kernel and the tile kernel derive for this case: XS, KP,
    nch, the FRONT predicate for the batch's largest K0, and the carves' own
    wide / KP / LDA for the batch's largest graph."""
    p = W.packed(family, f, out, batch)
    n, e, k0, p1, k1 = (int(a.max()) for a in p.sizes())
    sg = int(family == "sgat")
    xs, kp = W.r4(f), W.r16(2 * f)
    graph = _carve("fout", [n, e, f, k0, p1, k1, int(p.transpose_aliased), out, sg, LDS_MAX])
    conv = _carve("fout_conv", [n, f, k0, n, e, sg])  # (halo and tile edges bounded by the graph's)
    assert (graph["$XS"], graph["$KP"]) == (xs, kp)
    assert (conv["$XS"], conv["$KP"], conv["$LDA"]) == (xs, kp, kp + 4)
    assert 4 * graph["total"] <= LDS_MAX and 4 * conv["total"] <= LDS_MAX
    return {"XS": xs, "KP": kp, "nch": xs // 4, "k0": k0, "front": xs <= 32 and k0 <= 64, "wide": bool(graph["$wide"]), "pad_rows": kp - 2 * f}  # noqa: PLR2004


@pytest.mark.parametrize("family", ["foutnet", "sgat"])
def test_fout_widths_reach_every_layout_value(family):
    """Per-graph path: the widths and k0_over_64.  Tile + tail path: the widths
    alone, because it takes at most 64 depth-0 clusters (LargePlan refuses
    k0_over_64 before any launch; its conv kernel has no fused front, so the
    FRONT predicate is the per-graph kernel's only)."""
    per_graph = {c[1:]: _layout(*c) for c in FOUT_CASES if c[0] == family}
    large = {k: v for k, v in per_graph.items() if k[2] == "asym"}
    for lay in (per_graph, large):
        assert {v["nch"] for v in lay.values()} >= {1, 2, 8, 9, 16}
        assert {v["pad_rows"] == 0 for v in lay.values()} == {True, False}  # 2F == KP and 2F < KP
        assert {v["pad_rows"] for v in lay.values()} >= {0, 6, 8, 14}  # F = 8 / 32 / 64; 29; 4; 1 / 33
        assert {k[0] % 4 for k in lay} >= {0, 1}
        assert any(2 * k[0] < 16 for k in lay)  # noqa: PLR2004  (one k-step, mostly padding)
    assert {v["front"] for v in per_graph.values()} == {True, False}
    # FRONT false although r4(F) <= 32: the graph with more than 64 depth-0 clusters
    k0_case = per_graph[(*W.K0_OVER_64, "k0_over_64")]
    assert k0_case["XS"] <= 32 and k0_case["k0"] == 70 and not k0_case["front"] and k0_case["nch"] == 2  # noqa: PLR2004
    assert all(v["k0"] <= 64 for v in large.values())  # noqa: PLR2004
    # FRONT with chunks to drop (nch < 8: the guards ca < nch / cb < nch false) and without
    assert {v["nch"] for v in per_graph.values() if v["front"]} >= {1, 2, 8}
    # the non-front branch with idle lanes (nch < 8) and with more than one round (nch > 8)
    assert {v["nch"] for v in per_graph.values() if not v["front"]} >= {2, 9, 16}
    # Every case takes the wide [x | Zm] layout, and none of these batches can
    # take the narrow one: carve() goes narrow only when the wide carve exceeds
    # 160 KiB, and the widest case here (70 nodes, F = 64) needs about two
    # thirds of that.  The narrow layout is reached by a 265-node graph at
    # F = 30 in test_gpu_foutnet.py::test_foutnet_mixed_lds_layouts_vs_oracle.
    assert all(v["wide"] for v in per_graph.values())
    p = W.packed(family, 64, 14, "asym")
    n, e, k0, p1, k1 = (int(a.max()) for a in p.sizes())
    assert 4 * _carve("fout", [n, e, 64, k0, p1, k1, 0, 14, int(family == "sgat"), 1 << 30])["total"] < 3 * LDS_MAX // 4


def test_weight_image_fills_the_last_register_slot():
    assert W.image_words(64, 14) == 6142  # noqa: PLR2004
    assert max(W.image_words(f, out) for f, out in W.FOUT_WIDTHS) == 6142 <= 6144 < W.image_words(64, 15)  # noqa: PLR2004
    assert W.image_words(91, 1) > 6144 >= W.image_words(90, 1)  # noqa: PLR2004


def test_ginet_widths_sit_on_the_k_switch_and_the_limits():
    """GINet's kernels take K = 32 up to F = 32 and K = 64 beyond
    (``$KP`` of its carve); ginet_nocluster pads K to r16(F)."""
    kp = {f: _carve("ginet", [70, 600, f, 16, 60, 2, 0, out])["$KP"] for f, out in W.WIDTHS["ginet"]}
    assert kp == {1: 32, 32: 32, 33: 64, 64: 64}
    assert {W.r16(f) for f, _ in W.WIDTHS["nocluster"]} == {16, 32, 48, 64}
    assert {W.r16(f) - f for f, _ in W.WIDTHS["nocluster"]} >= {0, 15}
    assert max(out for ws in W.WIDTHS.values() for _, out in ws) == _lib.DR_MAX_OUT


@pytest.mark.parametrize("c", W.all_cases(), ids=IDS)
def test_batches_keep_transposed_arrays_apart(c):
    family, f, out, batch = c
    p = W.packed(*c)
    assert not p.transpose_aliased
    assert p.n_feat == f and p.n_graphs == (3 if batch == "k0_over_64" else 8)  # noqa: PLR2004
    n, _, k0, _, k1 = p.sizes()
    assert 30 <= n.min() and n.max() <= 70  # noqa: PLR2004
    if family != "nocluster":
        assert k1.max() == (5 if batch == "k0_over_64" else 2)  # noqa: PLR2004
        assert k0.max() == (70 if batch == "k0_over_64" else 16) and k0.min() >= 8  # noqa: PLR2004
    y = p.y[: p.n_graphs]
    if out > 1:
        np.testing.assert_array_equal(y, np.arange(p.n_graphs) % out)
    if family == "sgat":  # the one edge-feature column is the asymmetric batch's, divided by 6
        first = graph_zoo.asymmetric(fe=1, **graph_zoo.ASYM_BATCH)[0].edge_attr
        got = W.datas(*c)[0].edge_attr
        assert got.shape == first.shape and got.shape[1] == 1
        np.testing.assert_allclose(got.numpy() * 6.0, first.numpy(), rtol=1e-6)
        assert all(float(d.edge_attr.min()) > 0 for d in W.datas(*c))


@pytest.mark.parametrize("c", W.all_cases(), ids=IDS)
def test_fp64_oracle_is_finite_and_every_gradient_is_live(c):
    family = c[0]
    ref = W.oracle(*c)
    assert ref["out"].dtype == np.float64 and ref["out"].shape == (len(W.datas(*c)), c[2])
    assert np.isfinite(ref["out"]).all() and np.isfinite(ref["loss"])
    assert all(v.dtype == torch.float32 for v in ref["state"].values())  # what the HIP model loads
    assert (ref["mask"] is not None) == W.FAMILIES[family][2]
    for n, g in ref["grads"].items():
        assert g.dtype == np.float64 and np.isfinite(g).all(), n
        if W.is_zero_grad(family, n):  # the attention's singleton softmax (test_gpu_ginet.py:77)
            assert not np.any(g), n
        else:
            assert np.any(g), n
    if c[2] > 1:  # every fc2 row (output) has a gradient of its own
        assert np.abs(ref["grads"]["fc2.weight"]).max(axis=1).min() > 0


@pytest.mark.parametrize("c", W.all_cases(), ids=IDS)
def test_fp32_oracle_within_a_tenth_of_the_tolerance(c):
    """Condition on the inputs: if it fails for a new case, change that case's
    inputs (smaller degree, scaled edge weights), never this bound."""
    ref, ref32 = W.oracle(*c), W.oracle(*c, dtype=torch.float32)
    assert ref32["out"].dtype == np.float32
    for k, v in ref["state"].items():
        assert torch.equal(v, ref32["state"][k])
    r = W.ratios(ref32, ref)
    worst = max(r, key=r.get)
    print(f"[headroom {IDS(c)}] worst {worst} {r[worst]:.4f}")
    assert r[worst] <= HEADROOM, r
