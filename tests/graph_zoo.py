"""TEST INFRASTRUCTURE: graphs on which the transposed arrays of the store
differ from the forward ones, and graphs of degenerate size.

Every other whole-model test feeds doubled (symmetric) edges, where the packer
sets ``transpose_aliased`` and the kernels read ``col`` / ``p1`` for both
directions.  ``asymmetric`` builds batches whose node-level *and* pooled
adjacency are asymmetric; ``degenerate`` builds the smallest and the
tile-boundary graphs (N = 1, no edges, K0 = N, a hub row, N at and beside 16,
32, 64, 128).  Both return lists of ``oracle.pyg_ops.Data``.
"""

from __future__ import annotations

import numpy as np
import torch

from deeprank2_amd.utils.synthetic import connect_clusters, make_dataset
from oracle import data_ref
from oracle import pyg_ops as P

ASYM_BATCH = {"n": 8, "seed": 6, "frac": 0.6}  # the asymmetric batch of the CPU and GPU tests (test_store_topology.py says why)
ASYM_KW = {"n_lo": 30, "n_hi": 70, "mean_degree": 8.0, "k_lo": 8, "k_hi": 16}
BOUNDARY_N = (15, 16, 17, 32, 33, 63, 64, 65, 128, 129)
EDGELESS = (0, 2)  # positions of the graphs without edges in ``degenerate()``


def asymmetric(n, seed, frac, fe=3, **kw):
    """``n`` residue-size graphs with 8-16 depth-0 clusters each.  Of every
    graph's flipped edge copies (the second half of ``synthetic_to_data``'s
    edge list) a seeded random fraction ``frac`` is dropped; two self loops
    and one duplicated edge are appended; every second graph gets two depth-1
    clusters.  ``fe``: leading edge-feature columns kept (SGAT: 1).  ``kw``
    overrides ``make_dataset``'s arguments."""
    rng = np.random.default_rng(10007 * seed + 1)
    out = []
    for j, g in enumerate(make_dataset(n, seed=seed, **{**ASYM_KW, **kw})):
        d = data_ref.synthetic_to_data(g, f"asym{j}")
        ei, ea = d.edge_index.numpy(), d.edge_attr.numpy()
        half = ei.shape[1] // 2
        keep = np.ones(ei.shape[1], bool)
        keep[half + rng.choice(half, size=int(round(frac * half)), replace=False)] = False
        ei, ea = ei[:, keep], ea[keep]
        nn = d.x.shape[0]
        loops = rng.choice(nn, size=2, replace=False)
        dup = int(rng.integers(0, ei.shape[1]))
        ei = np.concatenate([ei, np.stack([loops, loops]), ei[:, dup : dup + 1]], axis=1)
        loop_ea = np.stack([rng.uniform(1.0, 4.0, size=2), np.ones(2), np.zeros(2)], axis=1).astype(np.float32)
        ea = np.concatenate([ea, loop_ea, ea[dup : dup + 1]])
        d.edge_index = torch.from_numpy(np.ascontiguousarray(ei))
        d.edge_attr = torch.from_numpy(np.ascontiguousarray(ea[:, :fe]))
        if j % 2:
            d.cluster1 = torch.tensor([k % 2 for k in range(len(d.cluster1))], dtype=torch.long)
        out.append(d)
    return out


def _graph(rng, n, pairs, cluster0, cluster1, name, directed=()):
    """A hand-made graph: ``pairs`` stored in both directions (pairs first,
    then their flipped copies, as the dataset does), ``directed`` edges once."""
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    one = np.asarray(directed, np.int64).reshape(-1, 2)
    ei = np.concatenate([pairs, pairs[:, ::-1], one]).T
    half = np.stack([rng.uniform(3.0, 9.0, size=len(pairs)), rng.integers(0, 2, size=len(pairs)), np.zeros(len(pairs))], axis=1)
    extra = np.stack([rng.uniform(3.0, 9.0, size=len(one)), np.ones(len(one)), np.zeros(len(one))], axis=1)
    ea = np.concatenate([half, half, extra]).astype(np.float32)
    d = P.Data(
        x=torch.from_numpy(rng.normal(size=(n, 30)).astype(np.float32)),
        edge_index=torch.from_numpy(np.ascontiguousarray(ei)).reshape(2, -1),
        edge_attr=torch.from_numpy(ea).reshape(-1, 3),
        y=torch.tensor([float(rng.uniform())]),
        pos=torch.from_numpy(rng.normal(size=(n, 3)).astype(np.float32)),
    )
    d.cluster0 = torch.as_tensor(np.asarray(cluster0), dtype=torch.long)
    d.cluster1 = torch.as_tensor(np.asarray(cluster1), dtype=torch.long)
    d.entry_names = name
    return d


def degenerate(fe=3, edgeless=True):
    """One batch (F = 30, Fe = 3) of: N = 1 (no edges); N = 2 (one undirected
    edge, two singleton clusters); N = 20 without edges (three clusters); a
    star of 40 nodes (hub row 0; four clusters, two depth-1 clusters); a ring
    of 24 nodes with directed chords i -> i + 5, every node its own depth-0
    cluster, three depth-1 clusters; and synthetic graphs of exactly
    ``BOUNDARY_N`` nodes.  ``edgeless=False`` leaves out the two graphs
    without edges (``EDGELESS``); ``fe``: leading edge-feature columns kept."""
    rng = np.random.default_rng(2024)
    ring = np.arange(24)
    out = [
        _graph(rng, 1, [], [0], [0], "one_node"),
        _graph(rng, 2, [(0, 1)], [0, 1], [0, 0], "one_edge"),
        _graph(rng, 20, [], np.arange(20) % 3, [0, 0, 0], "no_edges"),
        _graph(rng, 40, [(0, i) for i in range(1, 40)], np.arange(40) % 4, [0, 1, 0, 1], "star"),
        _graph(rng, 24, np.stack([ring, (ring + 1) % 24], 1), ring, ring % 3, "ring_chords", directed=np.stack([ring, (ring + 5) % 24], 1)),
    ]
    for n in BOUNDARY_N:
        (g,) = make_dataset(1, seed=500 + n, n_lo=n, n_hi=n, mean_degree=6.0, k_lo=2, k_hi=5)
        out.append(data_ref.synthetic_to_data(connect_clusters(g), f"n{n}"))
    assert [d.x.shape[0] for d in out[5:]] == list(BOUNDARY_N)
    if not edgeless:
        out = [d for i, d in enumerate(out) if i not in EDGELESS]
    for d in out:
        d.edge_attr = d.edge_attr[:, :fe].contiguous()
    return out


def batch(datas):
    """A fresh collated batch (the oracle's models modify theirs in place)."""
    return P.Batch.from_data_list([d.clone() for d in datas])
