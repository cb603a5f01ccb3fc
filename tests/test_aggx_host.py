"""Host-side contract of the store-wide ``Z = A x`` entries
(``dr_aggregate_x``, ``dr_ginet_graph_pass_z``, ``dr_ginet_acc_pass_z``,
``dr_ginet_z_lds_bytes``): sizes and argument checks, no GPU."""

from __future__ import annotations

import ctypes

import pytest

from deeprank2_amd import _lib

DR_E_ARG = -1
SIZES = (200, 3000, 30, 5, 20, 1)  # n, e, F, k0, p1, k1 (test_capi.py's residue graph)


@pytest.mark.parametrize("alias", [0, 1])
@pytest.mark.parametrize("stride", [34, 36])
def test_z_carve_is_smaller_than_the_gather_carve(alias, stride):
    lib = _lib.load()
    z = lib.dr_ginet_z_lds_bytes(*SIZES, alias, 1, stride)
    assert z > 0 and z % 16 == 0
    assert z < lib.dr_ginet_lds_bytes(*SIZES, alias, 1)
    # no x (N x r4(F)), no row pointers, no uint16 columns; Z rows at the given stride
    n, e, f = SIZES[:3]
    r4 = lambda v: (v + 3) & ~3  # noqa: E731
    saved = 4 * (r4(n * r4(f)) + r4(n + 1) + r4((e + 1) // 2) + r4(n * 34) - r4(n * stride))
    assert lib.dr_ginet_lds_bytes(*SIZES, alias, 1) - z == saved


def test_z_lds_bytes_refuses_a_stride_below_k():
    lib = _lib.load()
    assert lib.dr_ginet_z_lds_bytes(*SIZES, 1, 1, 30) < 0  # F = 30: K = 32
    assert lib.dr_ginet_z_lds_bytes(200, 3000, 40, 5, 20, 1, 1, 1, 36) < 0  # F = 40: K = 64


def _structs():
    st, w, p = _lib.GraphStoreC(), _lib.GinetWeightsC(), _lib.PassC()
    p.out_dim = 1
    p.flags = _lib.DR_PASS_FORWARD | _lib.DR_PASS_BACKWARD
    p.loss_kind = _lib.DR_LOSS_MSE
    st.n_graphs, st.n_feat, st.x_stride = 8, 30, 32
    return st, w, p


def test_z_pass_argument_checks_are_host_only():
    """A null ``z`` or a ``z_stride`` below the kernel's K (or odd: rows must
    stay 8-byte aligned) returns DR_E_ARG before anything touches the GPU."""
    lib = _lib.load()
    st, w, p = _structs()
    dummy = ctypes.c_void_p(16)  # never dereferenced: the checks return first
    sizes = (ctypes.c_int32 * 5)(200, 3000, 5, 20, 1)
    r = ctypes.byref
    for z, stride in [(None, 36), (dummy, 31), (dummy, 30), (dummy, 0), (dummy, 35)]:
        assert lib.dr_ginet_graph_pass_z(r(st), dummy, 8, r(w), r(p), 1024, z, stride, None) == DR_E_ARG, (z, stride)
        assert lib.dr_ginet_acc_pass_z(r(st), dummy, 8, r(w), r(p), 1024, 1024, 2, None, sizes, z, stride, None) == DR_E_ARG, (z, stride)
    st.n_feat, st.x_stride = 40, 40  # K = 64
    assert lib.dr_ginet_graph_pass_z(r(st), dummy, 8, r(w), r(p), 1024, dummy, 36, None) == DR_E_ARG
    assert lib.dr_ginet_acc_pass_z(r(st), dummy, 8, r(w), r(p), 1024, 1024, 2, None, sizes, dummy, 36, None) == DR_E_ARG


def test_aggregate_x_argument_checks_are_host_only():
    lib = _lib.load()
    st, _, _ = _structs()
    dummy = ctypes.c_void_p(16)
    assert lib.dr_aggregate_x(None, dummy, 36, 0, 8, None) == DR_E_ARG
    assert lib.dr_aggregate_x(ctypes.byref(st), None, 36, 0, 8, None) == DR_E_ARG
    assert lib.dr_aggregate_x(ctypes.byref(st), dummy, 29, 0, 8, None) == DR_E_ARG  # rows narrower than F
    assert lib.dr_aggregate_x(ctypes.byref(st), dummy, 36, 4, 5, None) == DR_E_ARG  # past the store's last graph
    assert lib.dr_aggregate_x(ctypes.byref(st), dummy, 36, 0, 0, None) == 0  # nothing to do
