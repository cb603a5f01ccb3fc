"""What the tile route of GINet integrated gradients
(``attribution.integrated_gradients(..., tiles=...)`` /
``dr_ginet_large_integrated_grad_pass``) settles without a device: the entry
and its struct are declared, every argument refusal of the C entry comes before
its first launch (the pointers handed in are never dereferenced), the Python
refusals and the routing of ``tiles=True`` around what the tile route does not
take, and the CPU reference the GPU test of the large batch compares with
(``ig_tiles_cases``): the fp32 oracle stays within a tenth of the tolerances of
the fp64 reference, so the whole budget is the kernel's."""

from __future__ import annotations

import ctypes
import inspect
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import ig_ref
import ig_tiles_cases
from deeprank2_amd import _lib, attribution
from deeprank2_amd.neuralnets.gnn.ginet import GINet

DR_OK, DR_E_ARG, DR_E_LDS, DR_E_UNSUPPORTED = 0, -1, -2, -3
DUMMY = 4096  # a 16-byte aligned address no check reads

# --------------------------------------------------------------------------
# the entry and the keyword exist
# --------------------------------------------------------------------------


def test_the_entry_is_declared_with_its_signature():
    names = [s[0] for s in _lib.SIGNATURES]
    assert names.count("dr_ginet_large_integrated_grad_pass") == 1
    assert _lib.load().dr_ginet_large_integrated_grad_pass.restype is ctypes.c_int
    # dz, z, part_key, part_val, part_arg | rows | zb_stride, pad
    assert ctypes.sizeof(_lib.IgTilesC) == 5 * 8 + 8 + 2 * 4
    assert ctypes.sizeof(_lib.LargePlanC) == 3 * 8 + 4 * 4 + 11 * 8  # dr_large_plan keeps its layout


def test_tiles_is_a_keyword_of_integrated_gradients_and_off_by_default():
    p = inspect.signature(attribution.integrated_gradients).parameters
    assert p["tiles"].default is None and p["tiles"].kind is inspect.Parameter.KEYWORD_ONLY
    assert attribution.TILES_DEFAULT is False
    assert isinstance(attribution.IG_TILE_GROUPS_DEFAULT, int) and attribution.IG_TILE_GROUPS_DEFAULT >= 1


# --------------------------------------------------------------------------
# integrated_gradients: refusals that need no device
# --------------------------------------------------------------------------


@pytest.mark.parametrize("tiles", ["yes", "forced", "", 1, 0, 2, 1.0, [True], ("force",)])
def test_other_values_of_tiles_are_refused_before_any_device(tiles):
    model = GINet(30, 1, 3)  # on the CPU: a call that got as far as the device check raises RuntimeError
    with pytest.raises(ValueError, match="tiles must be"):
        attribution.integrated_gradients(model, None, tiles=tiles)


@pytest.mark.parametrize("tiles", [None, False, True, "force"])
def test_the_four_values_of_tiles_pass_the_host_checks(tiles):
    with pytest.raises(RuntimeError, match="MI355X only"):  # the next refusal: the model is on the CPU
        attribution.integrated_gradients(GINet(30, 1, 3), None, tiles=tiles)


@pytest.mark.parametrize("tiles", [True, "force"])
def test_groups_outside_the_step_count_are_refused_with_tiles(tiles):
    for bad in (0, 9, -2, 1.0, True):
        with pytest.raises(ValueError, match="groups"):
            attribution.integrated_gradients(GINet(30, 1, 3), None, steps=8, groups=bad, tiles=tiles)


# --------------------------------------------------------------------------
# routing: what tiles=True sends to the layer route
# --------------------------------------------------------------------------


def _handle(nonfinite=False, k0=8, plan="a plan"):
    def large_plan(out_dim):
        if plan is None:
            msg = "large-graph path needs too much LDS"
            raise RuntimeError(msg)
        return plan

    return SimpleNamespace(nonfinite=nonfinite, max_sizes=(100, 600, k0, 12, 1), large_plan=large_plan)


def test_tile_checks_send_these_batches_to_the_layer_route():
    """``_tile_plan`` is the one gate of both tile routes: a bf16 store or
    ``fused=False`` (``kernel_ok`` off), a non-finite graph, more than 64
    clusters and a plan beyond one workgroup's LDS give no plan, and without a
    plan ``integrated_gradients`` takes the layer route whenever ``tiles`` is set."""
    ok, off = SimpleNamespace(kernel_ok=True, out_dim=2), SimpleNamespace(kernel_ok=False, out_dim=2)
    assert attribution._tile_plan(ok, _handle()) == "a plan"  # noqa: SLF001
    assert attribution._tile_plan(off, _handle()) is None  # noqa: SLF001
    assert attribution._tile_plan(ok, _handle(nonfinite=True)) is None  # noqa: SLF001
    assert attribution._tile_plan(ok, _handle(k0=attribution.K0_TILES_MAX + 1)) is None  # noqa: SLF001
    assert attribution._tile_plan(ok, _handle(k0=attribution.K0_TILES_MAX)) == "a plan"  # noqa: SLF001
    assert attribution._tile_plan(ok, _handle(plan=None)) is None  # noqa: SLF001
    route = attribution._route  # noqa: SLF001
    for fits in (True, False):
        assert route(True, None, fits) == route("force", None, fits) == "layers"  # the checks failed
    assert route(True, "a plan", False) == "tiles" and route(True, "a plan", True) == "fused"
    assert route("force", "a plan", False) == route("force", "a plan", True) == "tiles"
    assert route(False, None, True) == "fused" and route(False, None, False) == "layers"  # tiles off: as before


# --------------------------------------------------------------------------
# C entry: refusals before any launch
# --------------------------------------------------------------------------

_IG_PTRS = ("attr", "row_off", "alpha", "weight", "part", "part_off", "attr_sum", "slab", "head", "out")


def _args():
    """A set of arguments the entry accepts (n_batch = 0: DR_OK without a launch)."""
    st, w, p, pl = _lib.GraphStoreC(), _lib.GinetWeightsC(), _lib.PassC(), _lib.LargePlanC()
    ig, ws = _lib.IntegratedGradC(), _lib.IgTilesC()
    st.n_feat, st.x_stride = 30, 32
    st.x = st.t_rowptr = st.t_col = st.cl0 = DUMMY
    p.flags, p.out_dim, p.loss_kind, p.compute_dtype = _lib.DR_PASS_FORWARD | _lib.DR_PASS_BACKWARD, 2, _lib.DR_LOSS_NONE, _lib.DR_DTYPE_F32
    p.dout = DUMMY  # (slab, head and out are ig's)
    pl.tile_first = pl.z_row0 = pl.tile_slot = pl.z = pl.part_val = pl.part_arg = pl.part_key = DUMMY
    pl.n_tiles, pl.k0_max, pl.tile_rows = 8, 16, 64
    for k in _IG_PTRS:
        setattr(ig, k, DUMMY)
    ig.dx_stride, ig.n_steps, ig.n_groups, ig.part_rows = 32, 8, 3, 0
    ws.dz = ws.z = ws.part_key = DUMMY
    ws.rows, ws.zb_stride = 0, 36
    return dict(st=st, w=w, p=p, pl=pl, ig=ig, ws=ws, conv=64 * 1024, tail=64 * 1024, n=8)


def _call(a, null=()):
    ref = lambda k: None if k in null else ctypes.byref(a[k])  # noqa: E731
    return _lib.load().dr_ginet_large_integrated_grad_pass(ref("st"), DUMMY, a["n"], ref("pl"), ref("w"), ref("p"), ref("ig"), ref("ws"), a["conv"], a["tail"], None)


def _set(obj, **kw):
    for k, v in kw.items():
        setattr(obj, k, v)


def _plain(a):  # a plan without keys: the groups' partials are needed instead
    _set(a["pl"], part_key=None)
    _set(a["ws"], part_key=None, part_val=DUMMY, part_arg=DUMMY)


REFUSALS = {
    # the group workspaces
    "null ws": (lambda a: None, DR_E_ARG),
    "null dz": (lambda a: _set(a["ws"], dz=None), DR_E_ARG),
    "null z": (lambda a: _set(a["ws"], z=None), DR_E_ARG),
    "dz not 16-byte aligned": (lambda a: _set(a["ws"], dz=DUMMY + 8), DR_E_ARG),
    "z not 16-byte aligned": (lambda a: _set(a["ws"], z=DUMMY + 4), DR_E_ARG),
    "keys plan without group keys": (lambda a: _set(a["ws"], part_key=None, part_val=DUMMY, part_arg=DUMMY), DR_E_ARG),
    "plain plan without part_val": (lambda a: (_plain(a), _set(a["ws"], part_val=None)), DR_E_ARG),
    "plain plan without part_arg": (lambda a: (_plain(a), _set(a["ws"], part_arg=None)), DR_E_ARG),
    "negative rows": (lambda a: _set(a["ws"], rows=-1), DR_E_ARG),
    # what dr_ginet_integrated_grad_pass refuses
    "null ig": (lambda a: None, DR_E_ARG),
    "null store": (lambda a: None, DR_E_ARG),
    **{f"null {k}": ((lambda k: lambda a: _set(a["ig"], **{k: None}))(k), DR_E_ARG) for k in _IG_PTRS},
    "no steps": (lambda a: _set(a["ig"], n_steps=0), DR_E_ARG),
    "no groups": (lambda a: _set(a["ig"], n_groups=0), DR_E_ARG),
    "more groups than steps": (lambda a: _set(a["ig"], n_groups=9), DR_E_ARG),
    "attr not 16-byte aligned": (lambda a: _set(a["ig"], attr=DUMMY + 8), DR_E_ARG),
    "part not 16-byte aligned": (lambda a: _set(a["ig"], part=DUMMY + 4), DR_E_ARG),
    "dx_stride below F": (lambda a: _set(a["ig"], dx_stride=28), DR_E_ARG),
    "dx_stride not a multiple of 4": (lambda a: _set(a["ig"], dx_stride=34), DR_E_ARG),
    "negative part_rows": (lambda a: _set(a["ig"], part_rows=-1), DR_E_ARG),
    "zb without xb": (lambda a: _set(a["ig"], zb=DUMMY), DR_E_ARG),
    "xb without zb": (lambda a: _set(a["ig"], xb=DUMMY), DR_E_ARG),
    "zb not 16-byte aligned": (lambda a: _set(a["ig"], zb=DUMMY + 8, xb=DUMMY), DR_E_ARG),
    "zb_stride below r4(F)": (lambda a: (_set(a["ig"], zb=DUMMY, xb=DUMMY), _set(a["ws"], zb_stride=28)), DR_E_ARG),
    "zb_stride not a multiple of 4": (lambda a: (_set(a["ig"], zb=DUMMY, xb=DUMMY), _set(a["ws"], zb_stride=34)), DR_E_ARG),
    # what dr_ginet_large_input_grad_pass refuses
    "null pass": (lambda a: None, DR_E_ARG),
    "forward only": (lambda a: _set(a["p"], flags=_lib.DR_PASS_FORWARD), DR_E_ARG),
    "slot": (lambda a: _set(a["p"], slot=DUMMY), DR_E_ARG),
    "step_counter": (lambda a: _set(a["p"], step_counter=DUMMY), DR_E_ARG),
    "no t_rowptr": (lambda a: _set(a["st"], t_rowptr=None), DR_E_ARG),
    "no t_col": (lambda a: _set(a["st"], t_col=None), DR_E_ARG),
    "no cl0": (lambda a: _set(a["st"], cl0=None), DR_E_ARG),
    "bf16 compute": (lambda a: _set(a["p"], compute_dtype=_lib.DR_DTYPE_BF16), DR_E_UNSUPPORTED),
    # what dr_ginet_large_pass refuses
    "null plan": (lambda a: None, DR_E_ARG),
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
    "loss kind": (lambda a: _set(a["p"], loss_kind=99), DR_E_ARG),
}
_NULLS = {"null ws": "ws", "null ig": "ig", "null store": "st", "null pass": "p", "null plan": "pl"}


@pytest.mark.parametrize("case", list(REFUSALS))
def test_large_integrated_grad_pass_argument_checks_are_host_only(case):
    """Every refusal with a full batch (n_batch = 8) and dummy pointers: a
    check that came after a launch would touch them."""
    change, want = REFUSALS[case]
    a = _args()
    change(a)
    assert _call(a, null=(_NULLS[case],) if case in _NULLS else ()) == want


def test_an_empty_batch_is_ok_once_the_arguments_pass():
    a = _args()
    a["n"] = 0
    assert _call(a) == DR_OK
    _set(a["ig"], zb=DUMMY, xb=DUMMY)  # with a baseline
    assert _call(a) == DR_OK
    _set(a["ig"], n_steps=1, n_groups=1)
    assert _call(a) == DR_OK
    _set(a["ig"], n_steps=8, n_groups=8)
    assert _call(a) == DR_OK
    _plain(a)  # a plan without keys
    assert _call(a) == DR_OK
    _set(a["ws"], dz=None)
    assert _call(a) == DR_E_ARG  # the checks come first


def test_the_pass_buffers_of_the_caller_are_not_needed():
    """slab, head and out come from dr_integrated_grad (group g's rows); the pass's own may be NULL."""
    a = _args()
    a["n"] = 0
    assert not a["p"].slab and not a["p"].head and not a["p"].out
    assert _call(a) == DR_OK


# --------------------------------------------------------------------------
# the reference of the large batch, pinned on the CPU
# --------------------------------------------------------------------------


def test_the_large_batch_is_three_small_graphs_and_one_beyond_a_workgroup():
    ds = ig_tiles_cases.datas()
    n = [d.x.shape[0] for d in ds]
    assert len(ds) == 4 and n[ig_tiles_cases.LARGE_AT] == ig_tiles_cases.large_nodes() and max(n[:2] + n[3:]) <= 60
    q = _lib.load().dr_ginet_integrated_grad_lds_bytes
    big = ds[ig_tiles_cases.LARGE_AT]
    assert q(n[2], big.edge_index.shape[1], 30, 4, 12, 1, 1, 2, 36) > ig_tiles_cases.LDS_MAX
    for d in ds:  # no two nodes alike: the pools have no ties
        assert np.unique(d.x.numpy(), axis=0).shape[0] == d.x.shape[0]


@pytest.mark.parametrize("kind", ig_ref.BASELINES)
def test_fp32_oracle_stays_within_a_tenth_of_the_tolerance_of_the_fp64_reference_on_the_large_batch(kind):
    """8 Gauss-Legendre nodes, two outputs, target 1: every row of every graph
    is compared, with a tenth of the tolerances the GPU test applies in full."""
    ref, f32 = ig_tiles_cases.reference(kind), ig_tiles_cases.reference(kind, dtype=torch.float32)
    assert ref["attr"].dtype == np.float64 and f32["attr"].dtype == np.float32
    off = ref["node_off"]
    for k in ("out", "out_baseline"):
        assert (np.abs(f32[k] - ref[k]) <= 0.1 * (1e-4 + 1e-4 * np.abs(ref[k]))).all(), k
    assert np.array_equal(f32["seed"], ref["seed"])
    for g in range(len(off) - 1):
        rows = slice(off[g], off[g + 1])
        assert ig_ref.elementwise_excess(f32["attr"][rows], ref["attr"][rows]) <= 0.1, (kind, g)
        tol = ig_ref.sum_tolerance(ref, g)
        assert abs(f32["attr_sum"][g] - ref["attr_sum"][g]) <= 0.1 * tol and abs(f32["delta"][g] - ref["delta"][g]) <= 0.1 * tol
    assert np.abs(ref["attr"][off[2] : off[3]]).max() > 0
