"""bf16 GINet (``ginet_large_conv1_bf16_kernel`` / ``conv_tile_bf16`` and the
bf16 branch of ``tail_body``) against an oracle that rounds where the kernel
does (``oracle/bf16_ref.py``: x, Z = A x and W1 rounded to bf16, everything
else fp32), at the project's **fp32** tolerance: outputs rtol = atol = 1e-4,
loss 1e-4 relative, gradients through ``assert_grad_close``'s defaults, exact
zeros for the attention parameters, the fused Adam against ``torch.optim.Adam``.
``test_gpu_bf16.py`` keeps the comparison with the fp32 oracle at a bf16
tolerance; a wrong rounding point, a dropped K-pad column or a Z row from the
wrong slot passes there and fails here (``test_bf16_oracle.py`` proves the
latter on the CPU, through the same ``bf16_cases.assert_parity``).

Inputs (``bf16_cases.case``): 3-4 graphs of 60-200 nodes, 8-16 depth-0
clusters, three depth-1 clusters on every second graph, continuous x; every
input passes the tie guard (no pooled maximum within 1e-5 of its runner-up),
so an argmax cannot differ between the kernel and the oracle.  Of
``graph_zoo.degenerate()`` the star (all leaves share one Z row) and the
128-node graph (two pooled nodes with the same single neighbour) have exact
ties by construction and are left out, as the guard demands.

Reached here and by no other bf16 test: F outside 25..32 (non-zero Z pad
columns, XSB != KPB), two MFMA k-steps (F > 32), fewer and more than 8
chunks per row in the 8-lanes-per-row gather, the per-edge HBM gather
(``large_halos = False``), per-tile partial maxima (``large_atomic_max =
False``), tiles of 16 and 128 rows, graphs below one tile / at tile
boundaries / without edges / with K0 = N, and ``out_dim = 2``.

Measured on an MI355X (largest over all cases of this module; each test
prints its own figures, ``pytest -s``):

* bf16 kernel vs bf16 oracle: output error 5.2e-7 of max|out| (F = 20),
  normwise gradient error 7.3e-7 (F = 50);
* fp32 kernel vs fp32 oracle (``test_fp32_control_*``, same inputs): output
  error 6.9e-7 of max|out| (F = 20), normwise gradient error 1.2e-6 (F = 50).

Both sit at the fp32 summation-order floor, 100x under the tolerance, and
the figures are the same for every gather / combine / tile variant of a case
(the variants are bit-identical).  The stored Z rows matched bit for bit.
"""

from __future__ import annotations

import functools

import bf16_cases as C
import numpy as np
import pytest
import torch

from deeprank2_amd.engine import FusedTrainStep
from deeprank2_amd.fused import BatchHandle
from deeprank2_amd.neuralnets.gnn import ginet as amd
from deeprank2_amd.store import GraphStore, pack_graphs, records_from_batch
from oracle import gnn_ref
from oracle import pyg_ops as P

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ON_OFF = pytest.mark.parametrize("halos", [True, False], ids=["halos", "hbm_gather"])


@functools.lru_cache(maxsize=None)
def _store(key, dtype):
    datas = C.case(key)["datas"]
    return GraphStore(pack_graphs(records_from_batch(P.Batch.from_data_list([d.clone() for d in datas]))), DEV, dtype=dtype)


def _kernel_step(key, dtype="bf16", halos=True, atomic_max=True, tile=None):
    """One fused training step from the case's parameters; returns the
    comparison record, the step object, the batch handle and the parameters
    before the step."""
    c = C.case(key)
    C.assert_tie_guard(c["model"])
    m = amd.GINet(c["f"], c["out_dim"], 3)
    m.load_state_dict(c["state"])
    step = FusedTrainStep(m.to(DEV).train(), loss=c["loss"], compute_dtype=dtype)
    h = BatchHandle(_store(key, dtype), np.arange(len(c["datas"])))
    h.large_halos, h.large_atomic_max, h.large_tile = halos, atomic_max, tile
    before = [p.detach().clone() for p in step.params]
    loss, out = step.step(h, mask=c["mask"].to(torch.uint8).to(DEV))
    torch.cuda.synchronize()
    if dtype == "bf16":
        plan = h.large_plan(c["out_dim"], bf16=True)
        assert (plan.halo_tensors is not None) == halos and plan.TILE == (tile or 64)
    got = {"out": out.cpu().numpy().copy(), "loss": float(loss), "grads": {n: g.cpu().numpy().copy() for n, g in zip(amd.PARAM_NAMES, step.grads)}}
    return got, step, h, before


def _check_adam(step, before):
    """The fused Adam against torch.optim.Adam fed the kernel's gradients (test_gpu_ginet.py)."""
    ref = [torch.nn.Parameter(b) for b in before]
    for r, g in zip(ref, step.grads):
        r.grad = g.detach().clone()
    torch.optim.Adam(ref, lr=1e-3, weight_decay=1e-5).step()
    for n, r, p in zip(amd.PARAM_NAMES, ref, step.params):
        np.testing.assert_allclose(p.detach().cpu().numpy(), r.detach().cpu().numpy(), rtol=1e-5, atol=1e-7, err_msg=n)


def _parity(key, label, **knobs):
    got, step, _, before = _kernel_step(key, **knobs)
    C.assert_parity(got, C.case(key)["ref"], label=f"bf16 {label}")
    _check_adam(step, before)


@ON_OFF
@pytest.mark.parametrize("f", C.FEATURES)
def test_bf16_parity_feature_counts(f, halos):
    _parity(f, f"F={f} halos={halos}", halos=halos)


@ON_OFF
@pytest.mark.parametrize("tile", [16, 64, 128])
@pytest.mark.parametrize("f", [30, 33])
def test_bf16_parity_tile_sizes(f, tile, halos):
    _parity(f, f"F={f} tile={tile} halos={halos}", halos=halos, tile=tile)


@pytest.mark.parametrize("atomic_max", [True, False], ids=["atomic_max", "tile_partials"])
def test_bf16_parity_depth0_max_combine(atomic_max):
    _parity(33, f"F=33 atomic_max={atomic_max}", atomic_max=atomic_max, tile=16)  # 16-row tiles: 4-13 tiles per graph to combine


def test_bf16_parity_two_outputs_cross_entropy():
    _parity("ce", "out_dim=2 ce")


@ON_OFF
def test_bf16_parity_degenerate_batch(halos):
    c = C.case("degenerate")
    assert len(c["dropped"]) <= 2 and len(c["datas"]) >= 13  # noqa: PLR2004
    _parity("degenerate", f"degenerate halos={halos}", halos=halos)


@ON_OFF
@pytest.mark.parametrize("f", [30, 33])
def test_bf16_z_workspace_rows_bit_equal_to_oracle(f, halos):
    """The Z rows the tail reads for dW1, as the kernel stored them: at every
    node that is a depth-0 argmax of a positive maximum (either branch) the
    stored bf16 row equals the oracle's, bit for bit, over the F real columns.
    Checks the gather, the sum order, the rounding and the store address
    independently of everything downstream."""
    c = C.case(f)
    _, _, h, _ = _kernel_step(f, halos=halos)
    xsb = h.store.x_bf16_stride
    n_all = sum(d.x.shape[0] for d in c["datas"])  # graph b starts at row sum(n[:b]): the collated order
    z = h.large_plan(1, bf16=True).z.view(torch.int16)[: n_all * xsb].reshape(n_all, xsb).cpu().numpy().view(np.uint16)
    tr = c["model"].trace
    want = tr["z"].to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert torch.equal(tr["z"].to(torch.bfloat16).float(), tr["z"])  # the oracle's Z is bf16-representable
    nodes = set()
    for src, index in tr["pool0"]:
        best, arg = P.scatter_max(src, index, dim_size=int(index.max()) + 1)
        nodes |= set(arg[best > 0].tolist())
    nodes = np.array(sorted(nodes))
    assert nodes.size > 100 and nodes.max() < n_all  # noqa: PLR2004
    bad = nodes[(z[nodes, :f] != want[nodes]).any(axis=1)]
    assert bad.size == 0, f"{bad.size} of {nodes.size} stored Z rows differ from the oracle, first at nodes {bad[:8].tolist()}"


def test_bf16_bit_identical_across_gather_and_combine_variants():
    """Outputs, the slab-derived gradients and the head are bit-identical
    across (halos, atomic_max): the same sum order and MFMA chain whichever
    way the rows are fetched and the maxima combined (as
    test_gpu_large.py::test_large_path_bit_identical_to_single_workgroup_kernel
    for fp32)."""
    res = []
    for halos, amax in ((True, True), (False, True), (True, False), (False, False)):
        got, step, h, _ = _kernel_step(33, halos=halos, atomic_max=amax)
        res.append((got, step.slab[: h.B * amd.slab_stride(33)].cpu(), step.head[: h.B * amd.head_stride(1)].cpu()))
    for got, slab, head in res[1:]:
        assert np.array_equal(got["out"], res[0][0]["out"]) and got["loss"] == res[0][0]["loss"]
        assert torch.equal(slab, res[0][1]) and torch.equal(head, res[0][2])
        for n in amd.PARAM_NAMES:
            assert np.array_equal(got["grads"][n], res[0][0]["grads"][n]), n


@functools.lru_cache(maxsize=None)
def _fp32_reference(key):
    c = C.case(key)
    ref_model = gnn_ref.GINet(c["f"], c["out_dim"], 3)
    ref_model.load_state_dict(c["state"])
    return C.oracle_step(ref_model, c["datas"], c["mask"], c["loss"])


@pytest.mark.parametrize("key", [*C.FEATURES, "ce", "degenerate"])
def test_fp32_control_same_inputs_same_tolerance(key):
    """The fp32 kernel on the same inputs against ``gnn_ref.GINet`` through the
    same comparison: its printed error floor reads side by side with the bf16
    one (module docstring)."""
    got, step, _, before = _kernel_step(key, dtype="f32")
    C.assert_parity(got, _fp32_reference(key), label=f"fp32 control {key}")
    _check_adam(step, before)
