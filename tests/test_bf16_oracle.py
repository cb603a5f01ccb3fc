"""The bf16 GINet oracle (``oracle/bf16_ref.py``) checked on the CPU, and the
GPU parity test's comparison checked for sensitivity.

* With identity quantisers the oracle is ``gnn_ref.GINet``: pins the
  restructuring of ``scatter(fc(x[dst]))`` into ``(A x) W^T``.
* Its row sum is the sequential fp32 chain, bit for bit; its CSR order is the
  packer's; the kernel's ``f2bf`` formula gives torch's bf16 bits.
* The tie guard holds on every input the GPU parity tests use.
* Each single wrong rounding point (Z / W / x truncated, Z / W not rounded,
  one K column of Z dropped) trips ``bf16_cases.assert_parity``, the
  comparison the GPU tests apply.
"""

from __future__ import annotations

import bf16_cases as C
import graph_zoo
import numpy as np
import pytest
import torch
from _util import assert_grad_close

from deeprank2_amd.store import pack_graphs, records_from_batch
from oracle import bf16_ref, gnn_ref
from oracle import pyg_ops as P


def test_identity_quantisers_match_gnn_ref():
    """Duplicate edges, self loops, asymmetric adjacency, N = 1 and edgeless graphs."""
    datas = graph_zoo.asymmetric(n=3, seed=6, frac=0.6) + graph_zoo.degenerate()
    mask = C.dropout_mask(len(datas))
    torch.manual_seed(11)
    ref_model = gnn_ref.GINet(30, 1, 3)
    model = bf16_ref.GINetBf16(30, 1, 3, quant_x=bf16_ref.identity, quant_z=bf16_ref.identity, quant_w=bf16_ref.identity)
    model.load_state_dict(ref_model.state_dict())
    ref = C.oracle_step(ref_model, datas, mask)
    got = C.oracle_step(model, datas, mask)
    np.testing.assert_allclose(got["out"], ref["out"], rtol=1e-5, atol=1e-6)
    assert got["loss"] == pytest.approx(ref["loss"], rel=1e-5)
    for n, g in ref["grads"].items():
        if got["grads"][n] is None:  # conv1's attention parameters: no gradient here, exact zeros there
            assert n.startswith(("conv1.fc_", "conv1_ext.fc_")) and not np.any(g), n
            continue
        assert_grad_close(got["grads"][n], g, err_msg=n)
    assert sorted(n for n, g in got["grads"].items() if g is None) == sorted(f"{c}.{p}.weight" for c in ("conv1", "conv1_ext") for p in ("fc_attention", "fc_edge_attr"))


def test_sequential_row_sum_bit_equal_to_per_row_loop():
    rng = np.random.default_rng(3)
    n, f = 57, 13
    x = C.continuous_x(rng, n, f)
    rows = np.concatenate([rng.integers(0, n - 3, size=400), np.full(70, 5)])  # a hub row; rows n-3.. have no edge
    cols = rng.integers(0, n, size=rows.size)
    ei = torch.from_numpy(np.stack([rows, cols]))
    rowptr, col = bf16_ref.stable_csr(ei, n)
    got = bf16_ref.sequential_row_sum(x, rowptr, col).numpy()
    xn = x.numpy()
    want = np.zeros((n, f), np.float32)
    for e in range(rows.size):  # edge order within a row = stable-CSR order
        for k in range(f):
            want[rows[e], k] = np.float32(want[rows[e], k] + xn[cols[e], k])
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert not got[n - 3 :].any()
    # the chain order matters at this size: the reversed chain gives other bits somewhere
    rev = np.zeros((n, f), np.float32)
    for e in reversed(range(rows.size)):
        rev[rows[e]] = rev[rows[e]] + xn[cols[e]]
    assert not np.array_equal(rev, want)


@pytest.mark.parametrize("key", [*C.FEATURES, "ce", "degenerate"])
def test_csr_order_is_the_packers_and_inputs_pass_the_tie_guard(key):
    c = C.case(key)
    C.assert_tie_guard(c["model"])
    assert C.tie_guard(c["model"])[1] > 900  # noqa: PLR2004  (positive maxima the guard looked at)
    packed = pack_graphs(records_from_batch(P.Batch.from_data_list([d.clone() for d in c["datas"]])))
    for g, d in enumerate(c["datas"]):
        n = d.x.shape[0]
        rowptr, col = bf16_ref.stable_csr(d.edge_index, n)
        n0, e0, e1 = int(packed.node_off[g]), int(packed.edge_off[g]), int(packed.edge_off[g + 1])
        assert np.array_equal(packed.rowptr[n0 + g : n0 + g + n + 1], rowptr.numpy()), g
        assert np.array_equal(packed.col[e0:e1], col.numpy()), g
    if key == "degenerate":
        assert len(c["dropped"]) <= 2  # noqa: PLR2004
        names = [d.entry_names for d in c["datas"]]
        assert {"one_node", "one_edge", "no_edges", "ring_chords", "n64", "n65", "n129"} <= set(names)


def test_tie_guard_flags_exact_ties_and_tiny_maxima():
    """The star of ``graph_zoo.degenerate``: every leaf has the hub as its only
    neighbour, so all leaves share one Z row and every cluster's maximum is
    tied.  And a maximum far below max|H|."""
    datas = graph_zoo.degenerate()
    model = C.bf16_oracle(30, 1, 3)
    C.oracle_step(model, datas, C.dropout_mask(len(datas)))
    bad = C.tie_guard_failures(model)
    assert 3 in bad and any("runner-up" in s for s in bad[3])
    with pytest.raises(AssertionError, match="another seed"):
        C.assert_tie_guard(model)
    # tiny maximum: one cluster's only positive value at 1e-6 of the scale
    def failures(rows):
        h = torch.tensor(rows)
        model.trace = {"h1": [h], "h2": [], "pool0": [(torch.relu(h), torch.tensor([0, 1, 1]))], "pool1": [], "batch0": [torch.zeros(3, dtype=torch.long)], "batch1": []}
        return C.tie_guard_failures(model)

    bad = failures([[1.0, 2.0], [0.5, 1e-6], [0.0, -1.0]])
    assert list(bad) == [0] and len(bad[0]) == 1 and "below" in bad[0][0]
    assert not failures([[1.0, 2.0], [0.5, 0.3], [0.0, -1.0]])
    assert not failures([[1.0, 2.0], [0.5, 0.3], [0.5 * (1 - 2e-5), -1.0]])  # runner-up just outside the guard band
    bad = failures([[1.0, 2.0], [0.5, 0.3], [0.5 * (1 - 5e-6), -1.0]])  # and inside it
    assert len(bad[0]) == 1 and "runner-up" in bad[0][0]


def test_f2bf_formula_gives_torch_bf16_bits():
    bits = []
    for hi in (0x3F80, 0x3F81, 0x0001, 0x7F7E, 0x4049):  # even and odd bf16 mantissas
        for lo in (0x8000, 0x7FFF, 0x8001, 0x0000, 0x0001, 0xFFFF):  # exact half, just beside it, ends
            bits += [(hi << 16) | lo, 0x80000000 | (hi << 16) | lo]
    bits += [0x00000001, 0x00008000, 0x00007FFF, 0x00018000, 0x007FFFFF, 0x807FFFFF, 0x00400000]  # denormals
    bits += [0x00000000, 0x80000000, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F800000, 0xFF800000]  # +-0, largest finite, +-inf
    bits += [0x7FC00000, 0xFFC00000, 0x7F800001, 0x7FBFFFFF, 0xFF800001, 0x7FFFFFFF]  # quiet / signalling NaN
    rng = np.random.default_rng(0)
    bits += rng.integers(0, 2**32, size=4096, dtype=np.uint64).tolist()
    f = np.array(bits, dtype=np.uint64).astype(np.uint32).view(np.float32)
    got = bf16_ref.f2bf_bits(f)
    want = torch.from_numpy(f.copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    nan = np.isnan(f)
    assert np.array_equal(got[~nan], want[~nan])
    # NaN: torch's own bits depend on its code path (0x7fc0 from the scalar
    # conversion, 0xffff from the vectorised one), so there is no one pattern
    # to equal; both must be NaN, the formula's a quiet one with the sign kept
    assert got[bits.index(0x7FC00000)] == 0x7FC0 and got[bits.index(0x7F800001)] == 0x7FC0 and got[bits.index(0xFF800001)] == 0xFFC0
    assert np.all((got[nan] & 0x7FC0) == 0x7FC0) and np.all((want[nan] & 0x7F80) == 0x7F80) and np.all(want[nan] & 0x007F)
    assert np.array_equal(got[nan] >> 15, f[nan].view(np.uint32) >> 31)
    assert got[bits.index(0x7F7FFFFF)] == 0x7F80 and got[bits.index(0xFF7FFFFF)] == 0xFF80  # rounds to inf
    # and the oracle's quantiser is that rounding
    x = torch.from_numpy(f[~nan].copy())
    assert np.array_equal(bf16_ref.bf16_rne(x).numpy().view(np.uint32) >> 16, got[~nan].astype(np.uint32))


def _drop_column(k):
    def q(z):
        z = bf16_ref.bf16_rne(z).clone()
        z[:, k] = 0.0
        return z

    return q


MUTATIONS = {
    "z_truncated": {"quant_z": bf16_ref.bf16_trunc},
    "w_truncated": {"quant_w": bf16_ref.bf16_trunc},
    "x_truncated": {"quant_x": bf16_ref.bf16_trunc},
    "z_unrounded": {"quant_z": bf16_ref.identity},
    "w_unrounded": {"quant_w": bf16_ref.identity},
    "z_first_column_dropped": {"quant_z": _drop_column(0)},
    "z_last_column_dropped": {"quant_z": lambda z: _drop_column(z.shape[1] - 1)(z)},
}


@pytest.mark.parametrize("f", [12, 33])
@pytest.mark.parametrize("mutation", sorted(MUTATIONS))
def test_parity_comparison_notices_one_wrong_rounding_point(f, mutation):
    """The mutated oracle against the unmutated one, through the comparison of
    the GPU parity test: it must fail.  (Continuous x: ``bf16_cases.case``.)"""
    c = C.case(f)
    model = bf16_ref.GINetBf16(f, 1, 3, **MUTATIONS[mutation])
    model.load_state_dict(c["state"])
    got = C.oracle_step(model, c["datas"], c["mask"])
    with pytest.raises(AssertionError):
        C.assert_parity(got, c["ref"], label=f"{mutation} F={f}")
    # and the unmutated oracle, run again, passes it (the comparison is not simply always failing)
    again = bf16_ref.GINetBf16(f, 1, 3)
    again.load_state_dict(c["state"])
    C.assert_parity(C.oracle_step(again, c["datas"], c["mask"]), c["ref"], label=f"unmutated F={f}")
