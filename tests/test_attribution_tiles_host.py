"""What the tile route of the GINet input gradients
(``attribution.input_gradients(..., tiles=...)`` /
``dr_ginet_large_input_grad_pass``) refuses without a device: the values of
``tiles``, and the C entry's argument checks, which all come before its first
launch (the pointers handed in are never dereferenced)."""

from __future__ import annotations

import ctypes
import inspect

import pytest

from deeprank2_amd import _lib, attribution
from deeprank2_amd.neuralnets.gnn.ginet import GINet

DR_OK, DR_E_ARG, DR_E_LDS, DR_E_UNSUPPORTED = 0, -1, -2, -3
DUMMY = 4096  # a 16-byte aligned address no check reads


def test_tiles_default_is_off():
    assert attribution.TILES_DEFAULT is False
    assert inspect.signature(attribution.input_gradients).parameters["tiles"].default is None


@pytest.mark.parametrize("tiles", ["yes", "forced", "", 1, 0, 2, 1.0, [True], ("force",)])
def test_other_values_of_tiles_are_refused_before_any_device(tiles):
    model = GINet(30, 1, 3)  # on the CPU: a call that got as far as the device check raises RuntimeError
    with pytest.raises(ValueError, match="tiles must be"):
        attribution.input_gradients(model, None, tiles=tiles)


@pytest.mark.parametrize("tiles", [None, False, True, "force"])
def test_the_four_values_of_tiles_pass_the_host_checks(tiles):
    with pytest.raises(RuntimeError, match="MI355X only"):  # the next refusal: the model is on the CPU
        attribution.input_gradients(GINet(30, 1, 3), None, tiles=tiles)


def _args():
    """A set of arguments the entry accepts (n_batch = 0: DR_OK without a launch)."""
    st, w, p, pl, ig = _lib.GraphStoreC(), _lib.GinetWeightsC(), _lib.PassC(), _lib.LargePlanC(), _lib.InputGradC()
    st.n_feat, st.x_stride = 30, 32
    st.t_rowptr = st.t_col = st.cl0 = DUMMY
    p.flags, p.out_dim, p.loss_kind, p.compute_dtype = _lib.DR_PASS_FORWARD | _lib.DR_PASS_BACKWARD, 2, _lib.DR_LOSS_NONE, _lib.DR_DTYPE_F32
    p.out = p.dout = p.slab = p.head = DUMMY
    pl.tile_first = pl.z_row0 = pl.tile_slot = pl.z = pl.part_val = pl.part_arg = pl.part_key = DUMMY
    pl.n_tiles, pl.k0_max, pl.tile_rows = 8, 16, 64
    ig.dx, ig.row_off, ig.dx_stride = DUMMY, DUMMY, 32
    return dict(st=st, w=w, p=p, pl=pl, ig=ig, dz=DUMMY, conv=64 * 1024, tail=64 * 1024, n=8)


def _call(a, ig_null=False):
    ig = None if ig_null else ctypes.byref(a["ig"])
    return _lib.load().dr_ginet_large_input_grad_pass(ctypes.byref(a["st"]), DUMMY, a["n"], ctypes.byref(a["pl"]), ctypes.byref(a["w"]), ctypes.byref(a["p"]), ig, a["dz"], a["conv"], a["tail"], None)


def _set(obj, **kw):
    for k, v in kw.items():
        setattr(obj, k, v)


REFUSALS = {
    "null ig": (lambda a: None, DR_E_ARG),
    "null dx": (lambda a: _set(a["ig"], dx=None), DR_E_ARG),
    "null row_off": (lambda a: _set(a["ig"], row_off=None), DR_E_ARG),
    "null dz": (lambda a: a.update(dz=None), DR_E_ARG),
    "dx not 16-byte aligned": (lambda a: _set(a["ig"], dx=DUMMY + 4), DR_E_ARG),
    "dz not 16-byte aligned": (lambda a: a.update(dz=DUMMY + 8), DR_E_ARG),
    "dx_stride below F": (lambda a: _set(a["ig"], dx_stride=28), DR_E_ARG),
    "dx_stride not a multiple of 4": (lambda a: _set(a["ig"], dx_stride=34), DR_E_ARG),
    "forward only": (lambda a: _set(a["p"], flags=_lib.DR_PASS_FORWARD), DR_E_ARG),
    "slot": (lambda a: _set(a["p"], slot=DUMMY), DR_E_ARG),
    "step_counter": (lambda a: _set(a["p"], step_counter=DUMMY), DR_E_ARG),
    "no t_rowptr": (lambda a: _set(a["st"], t_rowptr=None), DR_E_ARG),
    "no t_col": (lambda a: _set(a["st"], t_col=None), DR_E_ARG),
    "no cl0": (lambda a: _set(a["st"], cl0=None), DR_E_ARG),
    "bf16 compute": (lambda a: _set(a["p"], compute_dtype=_lib.DR_DTYPE_BF16), DR_E_UNSUPPORTED),
    # what dr_ginet_large_pass refuses
    "negative batch": (lambda a: a.update(n=-1), DR_E_ARG),
    "out_dim": (lambda a: _set(a["p"], out_dim=_lib.DR_MAX_OUT + 1), DR_E_UNSUPPORTED),
    "n_feat": (lambda a: _set(a["st"], n_feat=65), DR_E_UNSUPPORTED),
    "conv LDS": (lambda a: a.update(conv=160 * 1024 + 4), DR_E_LDS),
    "tail LDS": (lambda a: a.update(tail=160 * 1024 + 4), DR_E_LDS),
    "plan without z": (lambda a: _set(a["pl"], z=None), DR_E_ARG),
    "plan without partials": (lambda a: _set(a["pl"], part_val=None), DR_E_ARG),
    "k0_max": (lambda a: _set(a["pl"], k0_max=65), DR_E_ARG),
    "tile_rows": (lambda a: _set(a["pl"], tile_rows=40), DR_E_ARG),
    "fewer tiles than graphs": (lambda a: _set(a["pl"], n_tiles=7), DR_E_ARG),
    "arrive": (lambda a: _set(a["pl"], arrive=DUMMY), DR_E_ARG),
    "no seed": (lambda a: _set(a["p"], dout=None), DR_E_ARG),
    "no slab": (lambda a: _set(a["p"], slab=None), DR_E_ARG),
    "loss kind": (lambda a: _set(a["p"], loss_kind=99), DR_E_ARG),
}


@pytest.mark.parametrize("case", list(REFUSALS))
def test_large_input_grad_pass_argument_checks_are_host_only(case):
    """Every refusal with a full batch (n_batch = 8) and dummy pointers: a
    check that came after a launch would touch them."""
    change, want = REFUSALS[case]
    a = _args()
    change(a)
    assert _call(a, ig_null=case == "null ig") == want


def test_an_empty_batch_is_ok_once_the_arguments_pass():
    a = _args()
    a["n"] = 0
    assert _call(a) == DR_OK
    _set(a["ig"], dx=None)
    assert _call(a) == DR_E_ARG  # the checks come first


def test_the_entry_is_declared_with_its_signature():
    names = [s[0] for s in _lib.SIGNATURES]
    assert names.count("dr_ginet_large_input_grad_pass") == 1
    assert _lib.load().dr_ginet_large_input_grad_pass.restype is ctypes.c_int
