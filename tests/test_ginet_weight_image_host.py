"""The lane-ordered image of GINet's conv1 B operands, checked on the host.

The KPT = 32 graph kernels stage ``[W1; W1e]`` (32 rows of F) as a 1 024-word
image whose word order is the order the MFMA lanes read it: four planes of 64
lanes x 4 words, lane ``l``'s registers ``4p .. 4p + 3`` at plane ``p``, words
``4l .. 4l + 3``.  Lane ``(li, kq) = (l & 15, l >> 4)`` holds in register ``r``
(``wa[r]`` for r < 8, ``wb[r - 8]`` else) the element at
``k = 16 * (j >> 2) + 4 * (j & 3) + kq``, ``j = r & 7``, of row ``li`` of W1
(``wa``) or W1e (``wb``), zero past F.

``dr_debug_ginet_w1_image`` (host only) returns the kernels' own index map
(image word -> element of the packed matrix, -1: zero) — the one the staging
DMA addresses its source with.  For every F in 1..32 it must be a bijection
onto the 32 F elements, zero elsewhere, and put each lane's registers where
the kernel's 16-byte reads fetch them.
"""

from __future__ import annotations

import ctypes

import numpy as np
import pytest

from deeprank2_amd import _lib

WORDS = 1024
DR_E_ARG = -1


def image_word(lane, r):
    """Word of the image that lane ``lane`` reads into register ``r`` (0..7 wa, 8..15 wb)."""
    return (r >> 2) * 256 + lane * 4 + (r & 3)


def image_table(F):
    lib = _lib.load()
    fn = lib.dr_debug_ginet_w1_image
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32]
    out = np.full(WORDS, -7, dtype=np.int32)
    assert fn(F, out.ctypes.data, WORDS) == 0
    return out


@pytest.mark.parametrize("F", range(1, 33))
def test_image_is_a_bijection_with_zero_padding(F):
    t = image_table(F)
    src = t[t >= 0]
    assert np.array_equal(np.sort(src), np.arange(32 * F)), "every element of [W1; W1e] exactly once"
    assert np.all(t[t < 0] == -1)
    assert int((t < 0).sum()) == WORDS - 32 * F


@pytest.mark.parametrize("F", range(1, 33))
def test_each_lane_register_gets_its_mfma_operand(F):
    t = image_table(F)
    seen = set()
    for lane in range(64):
        li, kq = lane & 15, lane >> 4
        for r in range(16):
            j = r & 7
            k = 16 * (j >> 2) + 4 * (j & 3) + kq
            row = li + (16 if r >= 8 else 0)  # packed rows 0..15: w1, 16..31: w1e
            w = image_word(lane, r)
            seen.add(w)
            assert t[w] == (row * F + k if k < F else -1), (F, lane, r)
    assert len(seen) == WORDS


def test_rejects_sizes_outside_the_image():
    lib = _lib.load()
    fn = lib.dr_debug_ginet_w1_image
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32]
    out = np.zeros(WORDS, dtype=np.int32)
    assert fn(0, out.ctypes.data, WORDS) == DR_E_ARG
    assert fn(33, out.ctypes.data, WORDS) == DR_E_ARG
    assert fn(30, out.ctypes.data, WORDS - 1) == DR_E_ARG
