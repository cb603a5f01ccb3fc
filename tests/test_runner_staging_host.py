"""Host side of what the captured runners share (``epoch.StagedBatches``,
``BatchHandle.fixed``): the two ``BatchHandle`` constructors agree on every
attribute and knob, and the staging arithmetic.  No GPU needed: the store sits
on the CPU."""

from __future__ import annotations

import functools

import numpy as np

from deeprank2_amd.epoch import StagedBatches
from deeprank2_amd.fused import VANILLA_CHUNK, BatchHandle
from deeprank2_amd.store import GraphRecord, GraphStore, pack_graphs
from deeprank2_amd.utils.synthetic import doubled_edges, make_dataset


@functools.lru_cache(maxsize=None)
def _store():
    recs = []
    for i, g in enumerate(make_dataset(3, seed=5, n_feat=30, n_lo=6, n_hi=9, mean_degree=3.0, k_lo=2, k_hi=3)):
        ei, ea = doubled_edges(g)
        recs.append(GraphRecord(x=g["x"], edge_index=ei, edge_attr=ea, cluster0=g["cluster0"], cluster1=g["cluster1"], y=float(g["y"]), name=f"g{i}"))
    return GraphStore(pack_graphs(recs), "cpu")


def test_fixed_handle_has_the_attributes_and_knobs_of_an_ordinary_one():
    """A knob added to one constructor only shows up here, not as an
    AttributeError on the captured path alone."""
    store = _store()
    ms = store.max_sizes(np.arange(3))
    fixed = BatchHandle.fixed(store, None, 2, ms)
    plain = BatchHandle(store, np.arange(2))
    assert set(vars(fixed)) == set(vars(plain))
    bare = BatchHandle.__new__(BatchHandle)
    bare._knob_defaults()  # noqa: SLF001
    knobs = set(vars(bare))
    assert {"_lds", "force_large", "large_tile", "large_halos", "large_atomic_max", "force_layers", "vanilla_words", "vanilla_split", "vanilla_tile_rows", "fault"} <= knobs
    for k in sorted(knobs):
        assert vars(fixed)[k] == vars(plain)[k] == vars(bare)[k], k
    assert fixed.vanilla_tile_rows == VANILLA_CHUNK
    # what makes it a fixed handle
    assert fixed.gids is None and fixed.descs is None and fixed.nonfinite is False
    assert fixed.B == 2 and fixed.max_sizes == ms  # noqa: PLR2004
    assert fixed.gids_host.dtype == np.int32 and fixed.gids_host.tolist() == [0, 0]


def test_staging_layout():
    offs, n, n_max, n_steps = StagedBatches.layout([[4, 4, 3], [2], []])
    assert [o.tolist() for o in offs] == [[0, 4, 8, 11], [0, 2], [0]]
    assert all(o.dtype == np.int64 for o in offs)
    assert (n, n_max, n_steps) == ([11, 2, 0], 11, 3)
    offs, n, n_max, n_steps = StagedBatches.layout([[5]])
    assert [o.tolist() for o in offs] == [[0, 5]]
    assert (n, n_max, n_steps) == ([5], 5, 1)
