"""Host-only checks of the GINet input-gradient path: the LDS query, every
argument refusal of ``dr_ginet_input_grad_pass`` (dummy pointers, no GPU), the
refusals of ``attribution.input_gradients`` that need no device, and the
batching / row-offset helper."""

from __future__ import annotations

import ctypes

import numpy as np
import pytest
import torch

from deeprank2_amd import _lib, attribution
from deeprank2_amd.neuralnets.gnn.ginet import GINet

LDS_MAX = 160 * 1024
r4 = lambda v: (v + 3) & ~3  # noqa: E731

# (n_nodes, n_edges, n_feat, k0, p1_edges, k1, transpose_aliased, out_dim)
SHAPES = [
    (200, 3000, 30, 5, 20, 1, 1, 1),
    (200, 3000, 30, 5, 20, 1, 0, 1),
    (1, 0, 30, 1, 0, 1, 1, 1),
    (24, 72, 30, 24, 96, 3, 0, 2),
    (70, 560, 33, 16, 90, 2, 0, 2),
    (129, 800, 12, 5, 20, 1, 1, 16),
]


def _stride(f):
    return (32 if f <= 32 else 64) + 4  # GraphStore.agg_x_stride


def test_lds_query_sizes():
    lib = _lib.load()
    q = lib.dr_ginet_input_grad_lds_bytes
    for s in SHAPES:
        n, e, f = s[:3]
        zs = _stride(f)
        gather, zform = q(*s, 0), q(*s, zs)
        assert gather > 0 and zform > 0
        assert gather % 16 == 0 and zform % 16 == 0
        # the gather form holds the transposed CSR where the forward CSR was; the Z form appends it
        assert gather == lib.dr_ginet_lds_bytes(*s)
        assert zform == lib.dr_ginet_z_lds_bytes(*s, zs) + 4 * (r4(n + 1) + r4((e + 1) // 2))
        assert zform >= lib.dr_ginet_z_lds_bytes(*s, zs)
    assert q(*SHAPES[0], 0) <= LDS_MAX and q(*SHAPES[0], 36) <= LDS_MAX
    assert q(*SHAPES[0], 16) == -1  # a Z stride below the kernel's K


def test_lds_query_is_monotone_in_nodes_and_edges():
    q = _lib.load().dr_ginet_input_grad_lds_bytes
    for zs in (0, 36):
        by_n = [q(n, 3000, 30, 5, 20, 1, 1, 1, zs) for n in range(1, 400, 7)]
        by_e = [q(200, e, 30, 5, 20, 1, 1, 1, zs) for e in range(0, 6000, 13)]
        assert all(a <= b for a, b in zip(by_n, by_n[1:])) and by_n[0] < by_n[-1]
        assert all(a <= b for a, b in zip(by_e, by_e[1:])) and by_e[0] < by_e[-1]


def _call(lib, dummy, *, flags=3, dtype=0, slot=None, step_counter=None, dx=16, row_off=16, dx_stride=32, ig_null=False, z=None, z_stride=0):
    """One dr_ginet_input_grad_pass call on an empty batch (n_batch = 0): the
    checks run before the batch size is looked at and nothing is launched."""
    st, w, p, ig = _lib.GraphStoreC(), _lib.GinetWeightsC(), _lib.PassC(), _lib.InputGradC()
    st.n_feat, st.x_stride = 30, 32
    p.flags, p.out_dim, p.loss_kind, p.compute_dtype = flags, 1, _lib.DR_LOSS_NONE, dtype
    p.out = p.dout = p.slab = p.head = dummy
    p.slot, p.step_counter = slot, step_counter
    ig.dx, ig.row_off, ig.dx_stride = dx, row_off, dx_stride
    return lib.dr_ginet_input_grad_pass(ctypes.byref(st), dummy, 0, ctypes.byref(w), ctypes.byref(p), None if ig_null else ctypes.byref(ig), z, z_stride, 1024, None)


def test_input_grad_pass_argument_checks_are_host_only():
    lib = _lib.load()
    dummy = ctypes.c_void_p(16)  # never dereferenced: the checks return first
    assert ctypes.sizeof(_lib.InputGradC) == 8 + 8 + 4 + 4
    assert _call(lib, dummy) == 0  # the accepted form (an empty batch: DR_OK without a launch)
    assert _call(lib, dummy, z=dummy, z_stride=36) == 0
    arg = [
        {"ig_null": True},
        {"dx": None},
        {"row_off": None},
        {"dx": 8},  # rows not 16-byte aligned
        {"dx_stride": 28},  # below F
        {"dx_stride": 34},  # not a multiple of 4
        {"slot": dummy},
        {"step_counter": dummy},
        {"flags": _lib.DR_PASS_FORWARD},  # no BACKWARD
        {"z": dummy, "z_stride": 16},  # a Z stride below the kernel's K
    ]
    for kw in arg:
        assert _call(lib, dummy, **kw) == -1, kw  # DR_E_ARG
    assert _call(lib, dummy, dtype=_lib.DR_DTYPE_BF16) == -3  # DR_E_UNSUPPORTED


def test_input_gradients_refusals_need_no_device():
    with pytest.raises(NotImplementedError, match="GINet"):
        attribution.input_gradients(torch.nn.Linear(30, 1), None)
    cpu1, cpu2 = GINet(30, 1, 3), GINet(30, 2, 3)
    with pytest.raises(RuntimeError, match="cuda"):
        attribution.input_gradients(cpu1, None)
    for bad in (2, -1, "best", 1.0, True):
        with pytest.raises(ValueError, match="target"):
            attribution.input_gradients(cpu2, None, target=bad)
    with pytest.raises(ValueError, match="target"):
        attribution.input_gradients(cpu2, None)  # two outputs and no target
    with pytest.raises(ValueError, match="not both"):
        attribution.input_gradients(cpu2, None, target=0, seed=torch.ones(1, 2))
    assert cpu1.training and cpu2.training  # refusals leave the flag alone


def test_reference_gradient_matches_central_differences():
    """The CPU reference the GPU tests compare with (attribution_ref: the
    oracle with a batch whose ``clone`` autograd follows) against central
    differences of the oracle's forward, at the entries of largest gradient;
    with the oracle's own deep-copying ``clone`` the second branch's share is
    missing, which this would catch (the entries differ by tens of percent)."""
    import attribution_ref  # noqa: PLC0415
    import graph_zoo  # noqa: PLC0415
    from oracle import gnn_ref  # noqa: PLC0415

    datas = graph_zoo.degenerate()[3:6]  # star, ring with chords, N = 15
    torch.manual_seed(11)
    model = gnn_ref.GINet(30, 2, 3).eval()
    _, g, seed, _ = attribution_ref.oracle_input_grad(model, datas, 1)
    x0 = graph_zoo.batch(datas).x

    def value(x):
        bat = graph_zoo.batch(datas)
        bat.x = x
        with torch.no_grad():
            return float((model(bat) * torch.from_numpy(seed)).sum())

    h = 1e-3
    flat = np.argsort(-np.abs(g).reshape(-1))[:12]
    for i, j in zip(*np.unravel_index(flat, g.shape)):
        xp, xm = x0.clone(), x0.clone()
        xp[i, j] += h
        xm[i, j] -= h
        fd = (value(xp) - value(xm)) / (2 * h)
        assert abs(fd - g[i, j]) <= 1e-3 + 0.05 * abs(g[i, j]), (i, j, fd, g[i, j])


def test_batch_rows_is_a_pure_layout_function():
    n_nodes = np.array([5, 1, 7, 3, 2])
    batches, off = attribution.batch_rows(n_nodes, [4, 0, 0, 2, 1], 2)
    assert batches == [(0, 2), (2, 4), (4, 5)]
    assert off.dtype == np.int64 and off.tolist() == [0, 2, 7, 12, 19, 20]
    batches, off = attribution.batch_rows(n_nodes, np.arange(5), 64)
    assert batches == [(0, 5)] and off.tolist() == [0, 5, 6, 13, 16, 18]
    batches, off = attribution.batch_rows(n_nodes, [], 3)
    assert batches == [] and off.tolist() == [0]
    for bad in ([5], [-1]):
        with pytest.raises(ValueError):
            attribution.batch_rows(n_nodes, bad, 2)
    with pytest.raises(ValueError):
        attribution.batch_rows(n_nodes, [0], 0)
    assert n_nodes.tolist() == [5, 1, 7, 3, 2]
