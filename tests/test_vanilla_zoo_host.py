"""The VanillaNetwork batches of tests/test_gpu_vanilla_zoo.py, on the CPU:
what that test claims of them holds, and it could tell if it did not.

From the packed arrays and ``vanilla_tile_plan`` on a CPU store, for every
batch of ``vanilla_zoo.BATCHES``:

* the transposed arrays differ from the forward ones (``transpose_aliased``
  false, ``t_col != col`` on every graph whose edge list is asymmetric);
* the 64-row tiles have the sizes recorded in ``vanilla_zoo.STATS``: below the
  2,048 items (256 halo rows) that the chunk kernels' prologues keep in
  registers for the ordinary batches, beyond them in the intended tiles of
  ``dense_tiles``, with no zero offset in its tile records;
* by the kernels' own carve functions (``dr_debug_carve_vanilla_*``) every
  batch expected on the chunk-fused kernels fits 160 KiB, ``hub_tiled`` keeps
  its tile plan but overflows a chunk carve, and ``hub_untiled`` overflows the
  tile carve itself, so ``vanilla_tile_plan`` returns None;
* the network restated in float64 on the planned arrays (columns and
  transposed sources read back through ``halo_ids`` / ``lcol`` / ``ltcol``)
  equals the float64 oracle, and with ``col`` read for ``t_col`` it misses the
  oracle's gradients by more than 100 times the widest GPU tolerance;
* the float32 oracle meets the project's tolerances against the float64
  oracle on every batch and loss, no entry left out (no ReLU gate of these
  batches sits within float32 rounding of zero in a way that shows).
"""

from __future__ import annotations

import numpy as np
import pytest

import vanilla_zoo as V
from deeprank2_amd.fused import LDS_MAX
from deeprank2_amd.neuralnets.gnn.vanilla_gnn import PARAM_NAMES

KPT_ITEMS = 2048  # vanilla_fused.hip: KPT * CT items per workgroup in registers, the rest by the tail loops
ALL = list(V.BATCHES)


@pytest.mark.parametrize("name", ALL)
def test_transposed_arrays_differ_from_forward(name):
    p = V.packed(name)
    assert not p.transpose_aliased
    hard = V.HARD.get(name)
    for g, d in enumerate(V.datas(name)):
        e = slice(int(p.edge_off[g]), int(p.edge_off[g + 1]))
        if V.is_symmetric(d):
            assert g != hard and name not in ("asym", *V.WIDTH_BATCHES)
            continue
        assert not np.array_equal(p.t_col[e], p.col[e]), g
    assert sum(not V.is_symmetric(d) for d in V.datas(name)) >= (2 if hard is not None else 1)


@pytest.mark.parametrize("name", ALL)
def test_tile_sizes_lie_where_the_gpu_test_claims(name):
    _, stats, meta = V.plan(name, lds_check=False)
    assert stats == V.STATS[name]
    n_tiles, hmax, emax, tmax = stats
    assert n_tiles == sum(-(-int(n) // V.CHUNK) for n in V.packed(name).sizes()[0]) == len(meta)
    if name.startswith("dense"):
        first = next(k for k, m in enumerate(meta) if m[7] == V.HARD[name])
        t0, t1, rest = meta[first], meta[first + 1], meta[first + 2 : first + 7]
        # (dr_vanilla_tile: ... 10 ne, 12 nq, 14 n_halo)
        assert t0[10] > KPT_ITEMS and t0[14] * 8 > KPT_ITEMS  # vc_fwd's record and halo tails, HaloV's
        assert t1[12] > KPT_ITEMS and t1[10] < KPT_ITEMS  # EdgeBwd's transposed-record tail alone
        assert all(m[10] < KPT_ITEMS and m[12] < KPT_ITEMS for m in rest)
        assert (emax, tmax) == (t0[10], t1[12]) and hmax == t0[14]
        for k, m in enumerate(meta[first : first + 7]):  # h0, lcol_off, ltcol_off, word0 and the row offsets; e0, q0 past the first tile
            assert all(m[j] > 0 for j in (0, 1, 2, 3, 4, 5, 13, 15, 16)), (k, m)
            assert k == 0 or (m[9] > 0 and m[11] > 0), (k, m)
    elif name.startswith("hub"):
        assert hmax == emax == getattr(V.graph_zoo, name.upper()) + 1  # the hub row's tile: its neighbours and one ordinary edge
    else:
        assert max(emax, tmax, 8 * hmax) < KPT_ITEMS
    if name == "deg" or name in V.HARD:  # a tile without a halo (the single node) beside tiles with one
        assert hmax > 0 and any(m[14] == 0 for m in meta)


@pytest.mark.parametrize("name", ALL)
def test_carves_put_every_batch_on_its_path(name):
    f, fe, _ = V.BATCHES[name]
    stats = V.STATS[name]
    c = V.carve_bytes(f, fe, *stats[1:])
    chunk = max(c["chunk_fwd"], c["chunk_eb2"], c["chunk_eb1"])
    tile = max(c["tile_fwd"], c["tile_bwd"])
    path = V.expected_path(f, fe, True, V.CHUNK, stats)
    assert path == V.PATHS[name]
    assert (V.plan(name) is None) == (tile > LDS_MAX)
    if path == "chunk":
        assert chunk <= LDS_MAX and tile <= LDS_MAX and f <= 32 and fe <= 4  # noqa: PLR2004
    if name == "hub_tiled":  # chunk_fused() falls back to the 64-row tiled edge kernels
        assert tile <= LDS_MAX < chunk
    if name == "hub_untiled":  # vanilla_tile_plan refuses: the untiled kernels
        assert tile > LDS_MAX and stats[1] <= 65535  # noqa: PLR2004
    if name in ("w40_3", "w64_8", "w30_5"):
        assert f > 32 or fe > 4  # noqa: PLR2004
    # the tiles of 16 rows and no tiles: the other kernels of the same batches
    assert V.expected_path(f, fe, True, 0, stats) == V.expected_path(f, fe, False, V.CHUNK, stats) == "untiled"
    if name in ("asym", "deg", "dense3", "dense4"):
        assert V.plan(name, 16) is not None
        assert V.expected_path(f, fe, True, 16, V.plan(name, 16)[1]) == "tiled"


@pytest.mark.parametrize("name", V.WIDTH_BATCHES)
def test_packed_weight_copy_only_within_the_per_graph_kernels_widths(name):
    """dr_vanilla_wpack packs for the per-graph kernel (F <= 32, Fe <= 4) and
    refuses wider models, which always run the pipeline: their spec offers
    FusedTrainStep no packed copy to keep current."""
    import ctypes

    from deeprank2_amd import _lib
    from deeprank2_amd.neuralnets.gnn.vanilla_gnn import make_spec

    f, fe, _ = V.BATCHES[name]
    wide = f > 32 or fe > 4  # noqa: PLR2004
    assert (make_spec(f, fe).wpack is None) == wide
    if wide:  # refused on the host, before any launch
        w, buf = _lib.VanillaWeightsC(), ctypes.create_string_buffer(16)
        assert _lib.load().dr_vanilla_wpack(w, f, fe, ctypes.addressof(buf), None) != 0


def _widest_tolerance(ref):
    return V.GRAD_CEILING * float(np.abs(ref).max()) + 1e-6 + V.GRAD_RTOL * np.abs(ref)


@pytest.mark.parametrize("tile_rows", [64, 16])
@pytest.mark.parametrize("name", ALL)
def test_restated_network_matches_oracle_and_shows_a_mixup(name, tile_rows):
    """The plan's ``lcol`` / ``ltcol`` lead back to ``col`` / ``t_col``; and a
    transposed sum that read ``col`` would be far outside what the GPU test
    tolerates at its widest (1e-5 max|ref| + rtol 1e-4)."""
    state, out_o, loss_o, grads_o = V.oracle(name, "mse", "f64")
    params = [state[n].numpy() for n in PARAM_NAMES]
    cols = V.planned_columns(name, tile_rows)
    out, loss, grads = V.restated(name, params, cols)
    np.testing.assert_allclose(out, out_o.reshape(-1), rtol=0, atol=1e-12)
    assert loss == pytest.approx(loss_o, rel=1e-12)
    for n in PARAM_NAMES:
        np.testing.assert_allclose(grads[n], grads_o[n], rtol=1e-9, atol=1e-12 * max(1.0, float(np.abs(grads_o[n]).max())), err_msg=n)
    _, _, mixed = V.restated(name, params, cols, swap=True)
    miss = max(float((np.abs(mixed[n] - grads_o[n]) / _widest_tolerance(grads_o[n])).max()) for n in PARAM_NAMES)
    assert miss > 100.0, miss  # noqa: PLR2004


@pytest.mark.parametrize(("name", "loss"), [(n, l) for n in ALL for l in V.LOSSES[n]])
def test_float32_oracle_meets_the_tolerances(name, loss):
    """Outputs rtol = atol = 1e-4, loss 1e-4 relative, gradients rtol 1e-4 with
    the floor max(1e-6, 1e-6 max|ref|): every entry."""
    _, out64, loss64, g64 = V.oracle(name, loss, "f64")
    _, out32, loss32, g32 = V.oracle(name, loss, "f32")
    np.testing.assert_allclose(out32, out64, **V.OUT_TOL)
    assert loss32 == pytest.approx(loss64, rel=V.LOSS_RTOL)
    for n in PARAM_NAMES:
        floor = max(1e-6, V.GRAD_NTOL * float(np.abs(g64[n]).max()))
        np.testing.assert_allclose(g32[n], g64[n], rtol=V.GRAD_RTOL, atol=floor, err_msg=n)
        atol, dev = V.grad_atol(g64[n], g32[n])
        assert floor <= atol <= max(floor, V.GRAD_CEILING * float(np.abs(g64[n]).max())) and atol <= max(floor, 4.0 * dev)
