"""Host-only checks of GINet integrated gradients: the quadrature, the LDS
query and carve, every argument refusal of ``dr_ginet_integrated_grad_pass``
(dummy pointers, no GPU), the refusals of ``attribution.integrated_gradients``
that need no device, and the CPU reference the GPU tests compare with
(``ig_ref``): the fp32 oracle stays within a tenth of the tolerance of the fp64
reference, so the whole budget is the kernel's, and the fp64 reference is
complete (``delta``) to 1e-2 of sum|attr| at 64 nodes."""

from __future__ import annotations

import ctypes

import numpy as np
import pytest
import torch

import ig_ref
from deeprank2_amd import _lib, attribution
from deeprank2_amd.neuralnets.gnn.ginet import GINet
from test_attribution_host import LDS_MAX, SHAPES, _stride, r4

# --------------------------------------------------------------------------
# quadrature
# --------------------------------------------------------------------------


@pytest.mark.parametrize("method", attribution.QUADRATURES)
@pytest.mark.parametrize("steps", [1, 2, 7, 8, 32, 64])
def test_quadrature_nodes_and_weights(method, steps):
    a, w = attribution.quadrature(method, steps)
    assert a.dtype == w.dtype == np.float64 and a.shape == w.shape == (steps,)
    assert abs(w.sum() - 1.0) <= 1e-15
    assert (a > 0).all() and (a < 1).all() and (np.diff(a) > 0).all() and (w > 0).all()
    if method == "gausslegendre":
        t, wt = np.polynomial.legendre.leggauss(steps)
        assert np.array_equal(a, 0.5 * (t + 1.0)) and np.array_equal(w, 0.5 * wt)
    else:
        assert np.array_equal(a, (np.arange(steps) + 0.5) / steps) and np.array_equal(w, np.full(steps, 1.0 / steps))


def test_quadrature_refusals():
    for bad in (0, -3, 1.5, True, None):
        with pytest.raises(ValueError, match="steps"):
            attribution.quadrature("midpoint", bad)
    with pytest.raises(ValueError, match="method"):
        attribution.quadrature("simpson", 8)


# --------------------------------------------------------------------------
# LDS query and carve
# --------------------------------------------------------------------------


def test_lds_query_sizes():
    lib = _lib.load()
    q = lib.dr_ginet_integrated_grad_lds_bytes
    for s in SHAPES:
        n, _, f = s[:3]
        zs = _stride(f)
        # the Z-form input-gradient layout, then the running dZ sum: N rows of r4(F) words
        assert q(*s, zs) == lib.dr_ginet_input_grad_lds_bytes(*s, zs) + 4 * r4(n * r4(f))
        assert q(*s, zs) % 16 == 0
        assert q(*s, (32 if f <= 32 else 64) - 4) == -1  # a Z stride below the kernel's K
        assert q(*s, 0) == -1  # no gather form
    assert q(*SHAPES[0], 36) <= LDS_MAX


def test_lds_query_is_monotone_in_nodes_and_edges():
    q = _lib.load().dr_ginet_integrated_grad_lds_bytes
    by_n = [q(n, 3000, 30, 5, 20, 1, 1, 1, 36) for n in range(1, 400, 7)]
    by_e = [q(200, e, 30, 5, 20, 1, 1, 1, 36) for e in range(0, 6000, 13)]
    assert all(a <= b for a, b in zip(by_n, by_n[1:])) and by_n[0] < by_n[-1]
    assert all(a <= b for a, b in zip(by_e, by_e[1:])) and by_e[0] < by_e[-1]


def _carve(kind, q):
    buf = ctypes.create_string_buffer(4096)
    n = getattr(_lib.load(), f"dr_debug_carve_{kind}")((ctypes.c_int32 * len(q))(*q), buf, 4096)
    assert 0 < n < 4096
    return {k: int(v) for k, v in (kv.split("=") for kv in buf.value.decode().strip(";").split(";"))}


@pytest.mark.parametrize("shape", SHAPES)
def test_carve_appends_the_dz_sum_behind_the_input_grad_layout(shape):
    """The pass never touches what lies behind its carve: the transposed CSR
    and dZacc start at the Z-form input-gradient layout's offsets and end."""
    n, e, f = shape[:3]
    q = [*shape, _stride(f)]
    ig, ours = _carve("ginet_ig", q), _carve("ginet_intgrad", q)
    assert all(ours[k] == v for k, v in ig.items() if k != "total")
    assert ours["trp"] == ours["$carve_total"] and ours["tcol"] == ours["trp"] + r4(n + 1)
    assert ours["dz"] == ig["total"] == ours["tcol"] + r4((e + 1) // 2)
    assert ours["dz"] % 4 == 0 and ours["total"] == ours["dz"] + r4(n * r4(f))
    assert 4 * ours["total"] == _lib.load().dr_ginet_integrated_grad_lds_bytes(*q)


# --------------------------------------------------------------------------
# C entry: refusals before any launch
# --------------------------------------------------------------------------

_PTRS = ("attr", "row_off", "alpha", "weight", "part", "part_off", "attr_sum", "slab", "head", "out")


def _call(lib, dummy, *, flags=3, dtype=0, slot=None, step_counter=None, ig_null=False, z=16, z_stride=36, store_null=False, **fields):
    """One dr_ginet_integrated_grad_pass call on an empty batch (n_batch = 0):
    the checks run before the batch size is looked at and nothing is launched."""
    st, w, p, ig = _lib.GraphStoreC(), _lib.GinetWeightsC(), _lib.PassC(), _lib.IntegratedGradC()
    st.n_feat, st.x_stride = 30, 32
    p.flags, p.out_dim, p.loss_kind, p.compute_dtype = flags, 1, _lib.DR_LOSS_NONE, dtype
    p.dout = dummy
    p.slot, p.step_counter = slot, step_counter
    for k in _PTRS:
        setattr(ig, k, 16)
    ig.dx_stride, ig.n_steps, ig.n_groups, ig.part_rows = 32, 8, 4, 0
    for k, v in fields.items():
        setattr(ig, k, v)
    return lib.dr_ginet_integrated_grad_pass(None if store_null else ctypes.byref(st), dummy, 0, ctypes.byref(w), ctypes.byref(p), None if ig_null else ctypes.byref(ig), z, z_stride, 1024, None)


def test_integrated_grad_pass_argument_checks_are_host_only():
    lib = _lib.load()
    dummy = ctypes.c_void_p(16)  # never dereferenced: the checks return first
    assert ctypes.sizeof(_lib.IntegratedGradC) == 8 + 8 + 4 * 4 + 4 * 8 + 8 + 8 + 8 + 8 + 3 * 8
    assert _call(lib, dummy) == 0  # the accepted form (an empty batch: DR_OK without a launch)
    assert _call(lib, dummy, zb=16, xb=16) == 0  # with a baseline
    assert _call(lib, dummy, n_steps=1, n_groups=1) == 0
    assert _call(lib, dummy, n_steps=8, n_groups=8) == 0
    arg = [
        {"ig_null": True},
        {"store_null": True},
        *({k: None} for k in _PTRS),
        {"n_steps": 0},
        {"n_groups": 0},
        {"n_groups": 9},  # more groups than steps
        {"attr": 8},  # rows not 16-byte aligned
        {"dx_stride": 28},  # below F
        {"dx_stride": 34},  # not a multiple of 4
        {"z": None},  # there is no gather form
        {"z_stride": 16},  # a Z stride below the kernel's K
        {"zb": 16},  # zb without xb
        {"xb": 16},  # xb without zb
        {"flags": _lib.DR_PASS_FORWARD},  # no BACKWARD
        {"slot": dummy},
        {"step_counter": dummy},
    ]
    for kw in arg:
        assert _call(lib, dummy, **kw) == -1, kw  # DR_E_ARG
    assert _call(lib, dummy, dtype=_lib.DR_DTYPE_BF16) == -3  # DR_E_UNSUPPORTED


# --------------------------------------------------------------------------
# integrated_gradients: refusals that need no device
# --------------------------------------------------------------------------


def test_integrated_gradients_refusals_need_no_device():
    ig = attribution.integrated_gradients
    with pytest.raises(NotImplementedError, match="GINet"):
        ig(torch.nn.Linear(30, 1), None)
    cpu1, cpu2 = GINet(30, 1, 3), GINet(30, 2, 3)
    with pytest.raises(RuntimeError, match="cuda"):
        ig(cpu1, None)
    for bad in (2, -1, "best", 1.0, True):
        with pytest.raises(ValueError, match="target"):
            ig(cpu2, None, target=bad)
    with pytest.raises(ValueError, match="target"):
        ig(cpu2, None)  # two outputs and no target
    with pytest.raises(ValueError, match="not both"):
        ig(cpu2, None, target=0, seed=torch.ones(1, 2))
    for bad in (0, -1, 2.5):
        with pytest.raises(ValueError, match="steps"):
            ig(cpu1, None, steps=bad)
    with pytest.raises(ValueError, match="method"):
        ig(cpu1, None, method="trapezoid")
    for bad in (0, 9, -2, 1.0, True):
        with pytest.raises(ValueError, match="groups"):
            ig(cpu1, None, steps=8, groups=bad)
    for bad in (torch.zeros(29), torch.zeros(5, 31), torch.zeros(2, 3, 30), 0.0):
        with pytest.raises(ValueError, match="baseline"):
            ig(cpu1, None, baseline=bad)
    assert cpu1.training and cpu2.training  # refusals leave the flag alone


def test_result_reads_as_input_gradients_do():
    attr = torch.arange(12.0).reshape(4, 3) - 5.0
    z = torch.zeros(2, 1)
    res = attribution.IntegratedGradients(attr, z, z, z, torch.zeros(2), torch.zeros(2), np.array([0, 1, 4]), np.array([7, 3]), "fused", np.ones(1, np.float32), np.ones(1, np.float32))
    assert res.dx is res.attr
    assert torch.equal(res.graph(1), attr[1:4]) and torch.equal(res.node_attr(), attr.sum(dim=1))
    assert torch.equal(attribution.node_scores(res, None, "l1"), attr.abs().sum(dim=1))
    assert attribution.top_nodes(res, attribution.node_scores(res, None, "l2"), 1, 2).tolist() == [2, 1]


# --------------------------------------------------------------------------
# the reference, pinned on the CPU
# --------------------------------------------------------------------------


@pytest.mark.parametrize("kind", ig_ref.BASELINES)
@pytest.mark.parametrize("batch", ig_ref.BATCHES)
def test_fp32_oracle_stays_within_a_tenth_of_the_tolerance_of_the_fp64_reference(batch, kind):
    """8 Gauss-Legendre nodes, two outputs, target 1: every row of every graph
    is compared, with a tenth of the tolerances the GPU tests apply in full."""
    ref, f32 = ig_ref.reference(batch, "t1", kind), ig_ref.reference(batch, "t1", kind, dtype=torch.float32)
    assert ref["attr"].dtype == np.float64 and f32["attr"].dtype == np.float32
    off = ref["node_off"]
    for k in ("out", "out_baseline"):
        assert (np.abs(f32[k] - ref[k]) <= 0.1 * (1e-4 + 1e-4 * np.abs(ref[k]))).all(), k
    assert np.array_equal(f32["seed"], ref["seed"])
    for g in range(len(off) - 1):
        rows = slice(off[g], off[g + 1])
        assert ig_ref.elementwise_excess(f32["attr"][rows], ref["attr"][rows]) <= 0.1, (batch, kind, g)
        tol = ig_ref.sum_tolerance(ref, g)
        assert abs(f32["attr_sum"][g] - ref["attr_sum"][g]) <= 0.1 * tol and abs(f32["delta"][g] - ref["delta"][g]) <= 0.1 * tol


@pytest.mark.parametrize("kind", ig_ref.BASELINES)
@pytest.mark.parametrize("batch", ig_ref.BATCHES)
def test_fp64_reference_is_complete_at_64_nodes(batch, kind):
    """Completeness: the attributions sum to (out - out_baseline) . seed up to
    the quadrature's error on fc1's and the pools' kinks."""
    ref = ig_ref.reference(batch, "t1", kind, steps=64)
    off = ref["node_off"]
    total = sum(np.abs(ref["attr"][off[g] : off[g + 1]]).sum() for g in range(len(off) - 1))
    assert np.abs(ref["delta"]).sum() <= 1e-2 * total
    assert total > 0
