"""The VanillaNetwork kernels (the batch-wide pipeline dr_vanilla_graph_pass
above all, and the per-graph kernel at its splits) on asymmetric, dense,
degenerate and odd-width batches, against ``oracle.gnn_ref.VanillaNetwork`` in
float64.

Every other pipeline test against a reference feeds doubled edges (``t_col``
and the plan's ``ltcol`` then equal ``col`` / ``lcol``), F = 30, Fe = 3 and
tiles far below the 2,048 items that the chunk kernels' prologues keep in
registers.  The batches here (``vanilla_zoo.BATCHES``; tests/
test_vanilla_zoo_host.py proves what is claimed of them on the CPU):

* ``asym`` / ``deg``: ``graph_zoo``'s asymmetric and degenerate batches
  (N = 1, graphs and tiles without edges, N at and beside 64 and 128) on the
  per-graph kernel with 1-4 workgroups per graph and on the pipeline with
  tiles of 64 (chunk-fused), 16 and 0 rows, with and without ReLU words, under
  MSE and 3-class CE;
* ``dense3`` / ``dense4``: a 64-row tile with 2,561 CSR edges and 399 halo
  rows, and one with 2,976 transposed edges: the prologue tail loops of
  vc_fwd, HaloV and EdgeBwd run (MapV's cannot: its item counts depend on F
  alone and end at 2,048 for F = 32);
* ``hub_tiled`` / ``hub_untiled``: one row of 1,000 / 1,200 edges; the first
  keeps its tile plan but overflows the chunk kernels' LDS (the 64-row tiled
  edge kernels run on buffers sized for the chunk-fused ones), the second
  overflows the tile carve (no plan: the untiled kernels);
* ``w<F>_<Fe>``: F in {12, 29, 32} x Fe in {0, 1, 4} chunk-fused, and
  (40, 3), (64, 8), (30, 5) beyond it.

Each case checks the forward output (rtol = atol = 1e-4), the in-kernel loss
(1e-4 relative), all 12 gradients (``vanilla_zoo.grad_atol``: the project's
rtol 1e-4 with the floor max(1e-6, 1e-6 max|ref|); where the float32 oracle
itself deviates more from float64, up to 4 x its deviation, never above 1e-5
max|ref|) and one Adam step against torch.optim.Adam fed the kernel's
gradients (rtol 1e-5 / atol 1e-7).  No tolerance is taken from a kernel's
output.

Measured on ``dense3`` (MSE, chunk-fused), largest absolute deviation from
the float64 oracle per gradient (max|ref|: float32 oracle / kernel):
  _external1._edge_mlp.0.weight  0.73:   1.9e-07 / 3.6e-07
  _external1._edge_mlp.0.bias    0.121:  3.1e-08 / 5.1e-08
  _external1._node_mlp.0.weight  0.657:  1.6e-07 / 2.0e-07
  _external1._node_mlp.0.bias    0.0562: 9.6e-09 / 8.3e-09
  _external2._edge_mlp.0.weight  0.759:  1.9e-07 / 2.0e-07
  _external2._edge_mlp.0.bias    0.124:  2.7e-08 / 3.3e-08
  _external2._node_mlp.0.weight  1.49:   4.7e-07 / 3.2e-07
  _external2._node_mlp.0.bias    0.0663: 1.3e-08 / 2.0e-08
  _graph_mlp.0.weight            0.67:   4.0e-07 / 1.6e-07
  _graph_mlp.0.bias              0.121:  1.4e-08 / 1.2e-08
  _graph_mlp.2.weight            3.06:   1.3e-06 / 6.1e-07
  _graph_mlp.2.bias              1.42:   1.1e-07 / 1.3e-07
Every one is inside the project's floor.  Over all cases the kernel's largest
deviation is 1.2 x the floor (hub_tiled, layer 2's edge-MLP weight: 1.2e-06 at
max|ref| 0.158, where the float32 oracle deviates by 2.6e-06).
"""

from __future__ import annotations

import numpy as np
import pytest
import torch
from _util import assert_same, dwc_mask

import vanilla_zoo as V
from vanilla_zoo import handle as _handle
from vanilla_zoo import train_step as _train_step
from deeprank2_amd import _lib
from deeprank2_amd.fused import LDS_MAX
from deeprank2_amd.neuralnets.gnn import vanilla_gnn as amd

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _assert_path(name, h):
    """Which kernels dr_vanilla_graph_pass ran for this handle, from the
    scratch struct it was given and the host carves: chunk_fused()'s rule
    (vanilla_fused.hip) restated, against ``vanilla_zoo.expected_path``."""
    f, fe, _ = V.BATCHES[name]
    tr = int(h.vanilla_tile_rows)
    c, _keep = h.vanilla_scratch(f, fe)
    stats = V.STATS[name] if tr == V.CHUNK else (V.plan(name, tr, lds_check=False)[1] if tr else None)
    want = V.expected_path(f, fe, h.vanilla_words, tr, stats)
    planned = bool(c.tile_row0) and c.n_tiles > 0
    if planned:
        assert (c.n_tiles, c.halo_max, c.tile_edges_max, c.tile_tedges_max) == stats
        carves = V.carve_bytes(f, fe, c.halo_max, c.tile_edges_max, c.tile_tedges_max)
        assert max(carves["tile_fwd"], carves["tile_bwd"]) <= LDS_MAX
        fits = max(carves["chunk_fwd"], carves["chunk_eb2"], carves["chunk_eb1"]) <= LDS_MAX
    chunk = planned and bool(c.tile_meta) and bool(c.relu_words) and c.tile_rows == V.CHUNK and c.part_layers == 2 and fe <= 4 and f <= 32 and c.n_tiles == c.n_chunks and fits  # noqa: PLR2004
    took = "chunk" if chunk else ("tiled" if planned and fe <= 4 else "untiled")  # noqa: PLR2004
    assert took == want, (took, want)
    return took


# --------------------------------------------------------------------------
# asymmetric and degenerate batches
# --------------------------------------------------------------------------


@pytest.mark.parametrize("loss", ["mse", "ce"])
@pytest.mark.parametrize("split", [1, 2, 3, 4])
@pytest.mark.parametrize("name", ["asym", "deg"])
def test_per_graph_kernel_splits_vs_float64_oracle(name, split, loss):
    """dr_vanilla_fused_pass with 1-4 workgroups per graph: graphs smaller
    than the split, graphs without edges and N at and beside 64 and 128 among
    them; no hand-off wait gives up and the arrival counters are left zero."""
    h = _train_step(name, loss, pipeline=False, vanilla_split=split)
    assert amd.fused_fits(h, 30, 3) and amd.split_k(h, 30, 3) == split
    sync = h.vanilla_fused_scratch()[2]
    assert h.vanilla_sync_ok(), "a hand-off wait gave up"
    assert int(sync.abs().sum()) == 0, "arrival counters not left zero"


@pytest.mark.parametrize("loss", ["mse", "ce"])
@pytest.mark.parametrize(("tile", "words"), [(64, True), (16, True), (0, True), (0, False)], ids=["chunk", "tile16", "untiled", "recomputed"])
@pytest.mark.parametrize("name", ["asym", "deg"])
def test_pipeline_vs_float64_oracle(name, tile, words, loss):
    """dr_vanilla_graph_pass on transposed arrays that differ from the forward
    ones, on tiles without a halo and on one-row last chunks: the chunk-fused
    kernels, the 16-row tiled edge kernels, the untiled kernels reading the
    forward's ReLU words and recomputing them."""
    h = _train_step(name, loss, vanilla_tile_rows=tile, vanilla_words=words)
    assert not amd.fused_fits(h, 30, 3) and amd.split_k(h, 30, 3) == 1
    assert _assert_path(name, h) == {64: "chunk", 16: "tiled", 0: "untiled"}[tile]


# --------------------------------------------------------------------------
# tiles beyond the prologues' registers, rows beyond a workgroup's LDS
# --------------------------------------------------------------------------


@pytest.mark.parametrize(("name", "tile", "loss"), [("dense3", 64, "mse"), ("dense3", 64, "ce"), ("dense4", 64, "mse"), ("dense3", 16, "mse"), ("dense4", 16, "mse"), ("dense3", 0, "mse"), ("dense4", 0, "mse")])
def test_dense_tiles_vs_float64_oracle(name, tile, loss):
    """More than 2,048 CSR edges and 256 halo rows in one 64-row tile, more
    than 2,048 transposed edges in the next: everything past the chunk
    kernels' two items per thread goes through their tail loops (Fe = 4: at
    twice the record stride).  The same graphs on 16-row tiles and untiled."""
    h = _train_step(name, loss, vanilla_tile_rows=tile)
    assert _assert_path(name, h) == {64: "chunk", 16: "tiled", 0: "untiled"}[tile]


@pytest.mark.parametrize("name", ["hub_tiled", "hub_untiled"])
def test_hub_row_takes_the_dispatch_fallbacks(name):
    """Default knobs (64-row tiles, ReLU words; the batch is beyond the
    per-graph kernel).  ``hub_tiled``: Python sized the partial buffer for the
    chunk-fused kernels (part_layers = 2, tile_meta), a chunk carve exceeds
    160 KiB and dr_vanilla_graph_pass runs the 64-row tiled edge kernels.
    ``hub_untiled``: the tile carve itself exceeds 160 KiB, vanilla_tile_plan
    returns None and the untiled kernels run."""
    h = _train_step(name, "mse", pipeline=False)
    assert not amd.fused_fits(h, 30, 3)
    c, _keep = h.vanilla_scratch(30, 3)
    assert c.part_layers == 2 and bool(c.relu_words)  # noqa: PLR2004
    assert (bool(c.tile_row0), bool(c.tile_meta)) == ((True, True) if name == "hub_tiled" else (False, False))
    assert _assert_path(name, h) == V.PATHS[name]


# --------------------------------------------------------------------------
# feature widths
# --------------------------------------------------------------------------


@pytest.mark.parametrize("fe", V.CHUNK_FE)
@pytest.mark.parametrize("f", V.CHUNK_F)
def test_chunk_fused_widths_vs_float64_oracle(f, fe):
    """F = 32 (no pad columns), F = 12 (r4(F) < 32: the guarded column
    pieces), F = 29 (three pad columns); Fe = 0 (a store without edge
    attributes), 1 and 4; a 130-node graph (two rows in its last chunk)."""
    name = f"w{f}_{fe}"
    h = _train_step(name, "mse")
    assert h.store.n_feat == f and h.store.n_edge_feat == fe
    assert _assert_path(name, h) == "chunk"


@pytest.mark.parametrize(("f", "fe"), V.UNFUSED_WIDTHS)
def test_unfused_widths_vs_float64_oracle(f, fe):
    """F > 32 (node GEMMs in two column halves, no chunk fusion, no per-graph
    kernel) and Fe > 4 (the generic edge kernels), default knobs."""
    name = f"w{f}_{fe}"
    h = _train_step(name, "mse", pipeline=False)
    assert not amd.fused_fits(h, f, fe)
    assert _assert_path(name, h) == V.PATHS[name] != "chunk"


# --------------------------------------------------------------------------
# 64-row chunk-fused tiles against no tiles, bit for bit
# --------------------------------------------------------------------------


@pytest.mark.parametrize("name", ["dense3", "dense4", "deg"])
def test_chunk_fused_bit_identical_to_untiled_on_hard_graphs(name):
    """vanilla_fused.hip promises the chunk-fused kernels the outputs, slab,
    head vectors and ReLU words of the untiled pipeline bit for bit (the
    slab's dWc entries, summed per tile first, at 1e-5 of their scale).

    ``out`` and ``slab`` enter filled with NaN: the pass writes every element
    of [B, out] and of its [B, DR_VANILLA_SLAB_STRIDE] slab rows, so an element
    it left out cannot compare equal.  ``head`` enters zeroed, as
    FusedFn.backward and FusedTrainStep hand it over: the pass leaves the pad
    entries of its dout and d mean vectors unwritten."""
    f, fe, _ = V.BATCHES[name]
    torch.manual_seed(18)
    m = amd.VanillaNetwork(f, 2, fe).to(DEV)
    b = V.packed(name).n_graphs
    written = b * (m.fused_spec.slab_stride(f) // amd.MAX_SPLIT)  # one partial row per graph on the pipeline
    res = []
    for tile in (V.CHUNK, 0):
        h = _handle(name, "ce", vanilla_pipeline=True, vanilla_tile_rows=tile)
        h.store.set_targets(np.arange(b) % 2)
        out = torch.full((b, 2), float("nan"), device=DEV)
        slab = torch.full((b * m.fused_spec.slab_stride(f),), float("nan"), device=DEV)
        head = torch.zeros(b * m.fused_spec.head_stride(2), device=DEV)
        amd.graph_pass(m, h, m.ordered_params(), 2, _lib.DR_PASS_FORWARD | _lib.DR_PASS_BACKWARD, loss_kind=_lib.DR_LOSS_CE, loss_scale=0.3, out=out, slab=slab, head=head)
        torch.cuda.synchronize()
        assert _assert_path(name, h) == ("chunk" if tile else "untiled")
        words = h.vanilla_scratch(f, fe)[1][4]
        res.append((out.cpu(), slab[:written].cpu(), head.cpu(), words.cpu()))
        assert all(bool(torch.isfinite(t).all()) for t in res[-1][:3])
    assert_same(res, dwc_mask(written, b, fe, F=f))
