"""The weight registers of GINet's graph kernels, dumped and compared exactly.

``dr_debug_ginet_weight_regs`` launches one workgroup that runs the staging and
loader helpers the graph kernels call (conv1's weights staged and read into the
MFMA B-operand registers ``wa`` / ``wb``; fc1.weight and fc1.bias in the row and
column register layouts of the head) and stores every thread's registers.  The weights are ``1 + flat index`` (exact in fp32), and
every register must *equal* the numpy-indexed element: these are moves.

F in {1, 3, 30, 32} runs the KPT = 32 kernel (the lane-ordered image: F not a
multiple of 4, the zero padding, the DMA's masked lanes), {33, 64} the KPT = 64
one (packed rows).
"""

from __future__ import annotations

import ctypes

import numpy as np
import pytest
import torch

from deeprank2_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NT, STRIDE = 1024, 49


def _arange(n, start, shape):
    return (start + torch.arange(n, dtype=torch.float32)).reshape(shape).to(DEV)


def _dump(F):
    lib = _lib.load()
    fn = lib.dr_debug_ginet_weight_regs
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.POINTER(_lib.GinetWeightsC), ctypes.c_int32, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]
    # distinct, exactly representable values in every matrix (all below 2^24)
    w1 = _arange(16 * F, 1, (16, F))
    w1e = _arange(16 * F, 1 + 16 * F, (16, F))
    fc1w = _arange(128 * 64, 5001, (128, 64))
    fc1b = _arange(128, 20001, (128,))
    w = _lib.GinetWeightsC()
    w.w1, w.w1e, w.fc1w, w.fc1b = w1.data_ptr(), w1e.data_ptr(), fc1w.data_ptr(), fc1b.data_ptr()
    out = torch.full((NT, STRIDE), -1.0, device=DEV)
    _lib.check(fn(ctypes.byref(w), F, out.data_ptr(), out.numel(), _lib.stream_ptr(torch.device(DEV))), "dr_debug_ginet_weight_regs")
    torch.cuda.synchronize()
    return out.cpu().numpy(), w1.cpu().numpy(), w1e.cpu().numpy(), fc1w.cpu().numpy(), fc1b.cpu().numpy()


@pytest.mark.parametrize("F", [1, 3, 30, 32, 33, 64])
def test_weight_registers_equal_the_indexed_elements(F):
    got, w1, w1e, fc1w, fc1b = _dump(F)
    t = np.arange(NT)
    j = np.arange(8)
    # fc1: row layout W[t >> 3][8 (t & 7) + j], column layout W[8 (t >> 6) + j][t & 63], bias[t >> 3]
    row = fc1w[(t >> 3)[:, None], (8 * (t & 7))[:, None] + j[None, :]]
    col = fc1w[(8 * (t >> 6))[:, None] + j[None, :], (t & 63)[:, None]]
    assert np.array_equal(got[:, 0:8], row)
    assert np.array_equal(got[:, 8:16], col)
    assert np.array_equal(got[:, 16], fc1b[t >> 3])
    # conv1 B operands: lane (li, kq), register j holds W[li][16 (j >> 2) + 4 (j & 3) + kq], zero past F
    nkv = 8 if F <= 32 else 16
    lane = t & 63
    li, kq = lane & 15, lane >> 4
    jj = np.arange(nkv)
    k = (16 * (jj >> 2) + 4 * (jj & 3))[None, :] + kq[:, None]
    inside = k < F
    kc = np.minimum(k, F - 1)
    wa = np.where(inside, w1[li[:, None], kc], np.float32(0))
    wb = np.where(inside, w1e[li[:, None], kc], np.float32(0))
    assert np.array_equal(got[:, 17 : 17 + nkv], wa)
    assert np.array_equal(got[:, 33 : 33 + nkv], wb)
    assert not got[:, 17 + nkv : 33].any() and not got[:, 33 + nkv :].any()
