"""Diagnostic: every LDS size and carve description of the large-graph path
(GINet, bf16 GINet, FoutNet / SGAT; tile kernels and tails) over the parameter
grid of tests/test_lds_carves.py, widened in F, one line each, to diff two
builds of the library (DR_LIB_NAME selects the build; host code only).

    DR_LIB_NAME=libdeeprank2_amd_<v>.so python tools/large_carves_dump.py > <v>.txt
"""

from __future__ import annotations

import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "deeprank-gnn-2_amd")]

from deeprank2_amd import _lib  # noqa: E402

FS = sorted({1, 8, 30, 32, 33, 50, 64})
CONV = [(3000, 32, 0, 0), (3000, 32, 600, 2400), (900, 8, 300, 1200), (16, 1, 16, 30), (2800, 16, 0, 0)]  # N, K0, HM, EM
TAIL = [(1, 0, 1, 1, 1), (32, 200, 1, 1, 2), (32, 200, 3, 0, 16), (32, 96, 2, 0, 2), (16, 48, 2, 0, 2)]  # K0, P1, K1, alias, OUT


def text(lib, kind, q):
    arr = (ctypes.c_int32 * len(q))(*q)
    buf = ctypes.create_string_buffer(8192)
    n = getattr(lib, f"dr_debug_carve_{kind}")(arr, buf, 8192)
    assert 0 < n < 8192  # noqa: PLR2004
    return buf.value.decode()


def main():
    lib = _lib.load()
    for N, K0, HM, EM in CONV:
        for F in FS:
            q = [N, F, K0, HM, EM]
            print("ginet_conv", q, lib.dr_ginet_large_conv_lds_bytes(*q), text(lib, "ginet_conv", q))
            print("ginet_conv_bf16", q, lib.dr_ginet_large_conv_lds_bytes_bf16(*q), text(lib, "ginet_conv_bf16", q))
            for sg in (0, 1):
                print("fout_conv", [*q, sg], lib.dr_fout_large_conv_lds_bytes(*q, sg), text(lib, "fout_conv", [*q, sg]))
    for q in TAIL:
        print("ginet_tail", list(q), lib.dr_ginet_tail_lds_bytes(*q), text(lib, "ginet_tail", list(q)))
        for sg in (0, 1):
            print("fout_tail", [*q, sg], lib.dr_fout_tail_lds_bytes(*q, sg), text(lib, "fout_tail", [*q, sg]))


if __name__ == "__main__":
    main()
