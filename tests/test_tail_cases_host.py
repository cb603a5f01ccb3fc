"""The cases of ``tail_cases.py`` are what they claim (host only): every batch
packs to the K0, K1, pooled rows and transposed rows its design names, the
transposed arrays are a copy of their own in the directed case alone, the row
degrees sit on both sides of the group sizes of ``ginet_tail``'s loops, the
fp64 oracle is finite with live gradients, and the fp32 oracle stays within a
tenth of the GPU comparison's tolerance of the fp64 one, so that comparison's
budget is the kernel's.
"""

from __future__ import annotations

import numpy as np
import pytest
import tail_cases as T
import torch
import width_cases as W

HEADROOM = 0.1  # of the GPU comparison's tolerance: a condition on the inputs, not a measurement
DESIGN_CASES = [(n, f) for n in T.DESIGNS for f in T.WIDTHS]


def _rows(rowptr, col, k00, g, q0, k0):
    rp = rowptr[k00 + g : k00 + g + k0 + 1]
    return [col[q0 + rp[k] : q0 + rp[k + 1]].tolist() for k in range(k0)]


@pytest.mark.parametrize("c", DESIGN_CASES, ids=lambda c: f"{c[0]}-F{c[1]}")
def test_batches_pack_to_the_pooled_graph_they_name(c):
    name, f = c
    k0, c1, _, directed = T.DESIGNS[name]
    p = T.packed(name, f, 1)
    assert p.n_graphs == T.GRAPHS and p.n_feat == f
    n, _, k0s, p1s, k1s = p.sizes()
    assert n.max() <= T.N_MAX
    assert k0s.tolist() == [k0] * T.GRAPHS and k1s.tolist() == [len(set(c1))] * T.GRAPHS
    assert bool(p.transpose_aliased) == (not directed)
    rows, trows = T.pooled_rows(name)
    assert p1s.tolist() == [sum(len(r) for r in rows)] * T.GRAPHS
    for g in range(T.GRAPHS):
        k00, q0 = int(p.k0_off[g]), int(p.p1_off[g])
        assert _rows(p.p1_rowptr, p.p1_col, k00, g, q0, k0) == rows  # no self loops, coalesced, sorted by (row, col)
        if directed:
            assert _rows(p.p1t_rowptr, p.p1t_col, k00, g, q0, k0) == trows
            assert trows != rows
        else:
            assert trows == rows
        assert max((len(r) for r in rows), default=0) <= max(k0 - 1, 0)
        # depth-1 members as designed
        k10 = int(p.k1_off[g])
        mp = p.m1_ptr[k10 + g : k10 + g + len(set(c1)) + 1]
        members = [sorted(p.m1_idx[k00 + mp[m] : k00 + mp[m + 1]].tolist()) for m in range(len(set(c1)))]
        assert members == [[k for k in range(k0) if c1[k] == m] for m in range(len(set(c1)))]


def test_designs_cover_the_group_sizes_and_the_switches():
    deg = {len(r) for name in T.DESIGNS for r in T.pooled_rows(name)[0]}
    tdeg = {len(r) for name in T.DESIGNS for r in T.pooled_rows(name)[1]}
    # conv2 forward takes 2 neighbours per group, the pooling backward 4:
    # empty rows, one short, full, one over, and several groups with and without a rest
    assert deg >= {0, 1, 2, 4, 5, 8, 9, 14, 15, 16}
    assert tdeg >= {0, 1, 2, 4, 5, 8, 9, 15, 16}
    k0s = {d[0] for d in T.DESIGNS.values()}
    assert k0s >= {1, 11, 12, 15, 16, 17}  # dW2 / dP1: direct | MFMA at 12; pooling: one cluster | general at 16
    assert {len(set(d[1])) for d in T.DESIGNS.values()} == {1, 2, 3}
    single = T.DESIGNS["k6_three_depth1_singleton"][1]
    assert min(single.count(m) for m in set(single)) == 1
    star = T.pooled_rows("k9_star")[0]
    assert sorted(len(r) for r in star) == [1] * 8 + [8]
    iso = T.pooled_rows("k5_isolated")[0]
    assert sorted(len(r) for r in iso) == [0, 2, 2, 2, 2]
    assert len(T.all_cases()) == 2 * (len(T.DESIGNS) + len(T.CE_CASES)) and set(T.CE_CASES) <= set(T.DESIGNS)


def test_hash_keep_flags_drop_and_keep():
    m = T.keep_mask()
    assert m.shape == (T.GRAPHS, 128) and 0.3 < float(m.mean()) < 0.9  # noqa: PLR2004
    assert set(np.unique(m.numpy()).tolist()) == {0.0, 1.0}


@pytest.mark.parametrize("c", T.all_cases(), ids=T.case_id)
def test_fp64_oracle_is_finite_and_every_gradient_is_live(c):
    ref = T.oracle(*c)
    assert ref["out"].dtype == np.float64 and ref["out"].shape == (T.GRAPHS, c[2])
    assert np.isfinite(ref["out"]).all() and np.isfinite(ref["loss"])
    assert all(v.dtype == torch.float32 for v in ref["state"].values())  # what the HIP model loads
    # K0 = 1: no pooled edge, so conv2 sums nothing, H2 = 0 and the gradient
    # reaches the head's biases and fc2.weight (through relu(fc1.bias)) alone
    no_edge = T.DESIGNS[c[0]][0] == 1
    for n, g in ref["grads"].items():
        assert g.dtype == np.float64 and np.isfinite(g).all(), n
        if W.is_zero_grad("ginet", n) or (no_edge and n not in ("fc1.bias", "fc2.weight", "fc2.bias")):
            assert not np.any(g), n
        else:
            assert np.any(g), n


@pytest.mark.parametrize("c", T.all_cases(), ids=T.case_id)
def test_fp32_oracle_within_a_tenth_of_the_tolerance(c):
    """Condition on the inputs: if it fails for a new case, change that case's
    inputs, never this bound."""
    ref, ref32 = T.oracle(*c), T.oracle(*c, dtype=torch.float32)
    assert ref32["out"].dtype == np.float32
    for k, v in ref["state"].items():
        assert torch.equal(v, ref32["state"][k])
    r = W.ratios(ref32, ref)
    worst = max(r, key=r.get)
    print(f"[headroom {T.case_id(c)}] worst {worst} {r[worst]:.4f}")
    assert r[worst] <= HEADROOM, r
