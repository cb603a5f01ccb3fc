"""``vanilla_graph_kernel<FE>`` (dr_vanilla_fused_pass, the default Vanilla path
for residue-size graphs) at the feature widths on which its code branches,
against ``oracle.gnn_ref.VanillaNetwork`` in float64.

Every other comparison of this kernel with a reference runs F = 30 (x rows of
32 floats, Nn = F + 33 = 63, two row tiles), Fe in 1..4 and at most 3 outputs;
the ``w<F>_<Fe>`` batches of test_gpu_vanilla_zoo.py go to the pipeline.  Here
the same batches (``graph_zoo.widths``: three asymmetric graphs of 30-70 nodes
and one of 130, transposed arrays that differ from the forward ones) run on the
per-graph kernel at ``vanilla_zoo.PER_GRAPH_WIDTHS`` (test_vanilla_zoo_host.py
proves on the CPU that they fit, that the x rows are r4(F) floats and that
every gradient is live):

* the nine chunk widths {12, 29, 32} x {0, 1, 4};
* (1, 0), (1, 3): every ``min(.., M - 1)`` / ``min(.., Nn - 1)`` clamp at 0;
* (4, 2): x rows of 4 floats (the layer-1 backward re-stages X0 at that
  stride, not the slots' 34);
* (15, 1), (16, 4), (17, 2): F + 33 = 48 | 49 | 50 (three | four column tiles
  of the weight-gradient GEMMs), the packed row-pass block's upper half all
  zero up to 16 and live from 17 on, one | two row tiles, x rows of 20;
* (31, 3), (32, 2): F + 33 = 64 | 65, no pad column at 32;
* FE = 0: a store without edge attributes; FE = 4: the 8-word records at a
  narrow F;

each with 1 and 4 workgroups per graph ((17, 2), (1, 3) and (32, 2) with 2 and
3 as well), and ``deg17_2``, the degenerate batch at (17, 2), whose one- and
two-node graphs leave siblings without a row.  Further: 16 (= DR_MAX_OUT)
classes through the head at (12, 0) and (32, 4), per-graph and on the
chunk-fused pipeline; a forward-only pass, whose outputs equal the training
pass's bit for bit and which leaves the arrival counters zero; and two runs of
one split case, bit for bit.

Checks and tolerances are test_gpu_vanilla_zoo.py's (``vanilla_zoo.train_step``):
outputs rtol = atol = 1e-4, loss 1e-4 relative, all 12 gradients under
``vanilla_zoo.grad_atol``, one Adam step against torch.optim.Adam at rtol 1e-5
/ atol 1e-7.  Each case also holds that the intended kernel ran: the batch fits
it, the split is the one asked for, no hand-off wait gave up and the arrival
counters are left zero.
"""

from __future__ import annotations

import numpy as np
import pytest
import torch
import vanilla_zoo as V
from test_gpu_vanilla_zoo import _assert_path

from deeprank2_amd import _lib
from deeprank2_amd.neuralnets.gnn import vanilla_gnn as amd

pytestmark = pytest.mark.gpu
DEV = V.DEV
EVERY_SPLIT = ((17, 2), (1, 3), (32, 2))
CASES = [(f, fe, k) for f, fe in V.PER_GRAPH_WIDTHS for k in ((1, 2, 3, 4) if (f, fe) in EVERY_SPLIT else (1, 4))]


def _assert_per_graph_kernel_ran(h, f, fe, k):
    assert h.store.n_feat == f and h.store.n_edge_feat == fe and h.store.x_stride == (f + 3) & ~3
    assert amd.fused_fits(h, f, fe) and amd.split_k(h, f, fe) == k
    sync = h.vanilla_fused_scratch()[2]
    assert h.vanilla_sync_ok(), "a hand-off wait gave up"
    assert int(sync.abs().sum()) == 0, "arrival counters not left zero"


@pytest.mark.parametrize(("f", "fe", "k"), CASES, ids=[f"F{f}-Fe{fe}-k{k}" for f, fe, k in CASES])
def test_per_graph_kernel_widths_vs_float64_oracle(f, fe, k):
    h = V.train_step(f"w{f}_{fe}", "mse", pipeline=False, vanilla_split=k)
    _assert_per_graph_kernel_ran(h, f, fe, k)


@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_siblings_without_rows_at_another_width(k):
    """``deg17_2``: graphs of 1 and 2 nodes, and graphs without edges, at
    F = 17, Fe = 2 (test_vanilla_zoo_host.py: siblings own no row there)."""
    h = V.train_step("deg17_2", "mse", pipeline=False, vanilla_split=k)
    _assert_per_graph_kernel_ran(h, 17, 2, k)


@pytest.mark.parametrize("path", ["k1", "k4", "chunk"])
@pytest.mark.parametrize("name", V.CE16)
def test_sixteen_classes_vs_float64_oracle(name, path):
    """``out_dim`` = DR_MAX_OUT: 16 logits fill the per-graph kernel's ``sdout``
    exactly (``sdm`` starts right behind it), and the pipeline's head kernel
    takes as many; cross entropy with targets i % 16."""
    f, fe, _ = V.BATCHES[name]
    assert _lib.DR_MAX_OUT == 16  # noqa: PLR2004
    if path == "chunk":
        h = V.train_step(name, "ce", pipeline=True, out_dim=16)
        assert not amd.fused_fits(h, f, fe) and _assert_path(name, h) == "chunk"
    else:
        h = V.train_step(name, "ce", pipeline=False, out_dim=16, vanilla_split=int(path[1]))
        _assert_per_graph_kernel_ran(h, f, fe, int(path[1]))


@pytest.mark.parametrize("k", [1, 4])
@pytest.mark.parametrize(("f", "fe"), [(12, 0), (17, 2)])
def test_forward_only_pass_equals_the_training_pass(f, fe, k):
    """DR_PASS_FORWARD alone: the kernel returns after the head's outputs (a
    split graph's siblings leave through ``sib_exit`` at their last hand-off),
    the outputs are the training pass's bit for bit and the arrival counters
    are zero afterwards.  ``out`` enters filled with NaN."""
    name = f"w{f}_{fe}"
    got = {}
    V.train_step(name, "mse", pipeline=False, got=got, vanilla_split=k)
    h = V.handle(name, "mse", vanilla_split=k)
    m = amd.VanillaNetwork(f, 1, fe)
    m.load_state_dict(V.oracle(name, "mse", "f64")[0])
    m = m.to(DEV).eval()
    out = torch.full((h.B, 1), float("nan"), device=DEV)
    for _ in range(2):  # (the second launch starts from the counters the first one left)
        amd.graph_pass(m, h, m.ordered_params(), 1, _lib.DR_PASS_FORWARD, out=out)
        torch.cuda.synchronize()
        _assert_per_graph_kernel_ran(h, f, fe, k)
        assert np.array_equal(out.cpu().numpy(), got["out"])


def test_split_case_is_bit_repeatable():
    """(4, 2) with 4 workgroups per graph, twice from the same parameters:
    outputs, loss and all 12 gradients identical (fixed summation orders: the
    siblings' partial rows and column sums combine in sibling order)."""
    runs = [{}, {}]
    for got in runs:
        h = V.train_step("w4_2", "mse", pipeline=False, got=got, vanilla_split=4)
        _assert_per_graph_kernel_ran(h, 4, 2, 4)
    a, b = runs
    assert np.array_equal(a["out"], b["out"]) and a["loss"] == b["loss"]
    for n in amd.PARAM_NAMES:
        assert np.array_equal(a["grads"][n], b["grads"][n]), n
