"""TEST INFRASTRUCTURE: graphs on which the transposed arrays of the store
differ from the forward ones, and graphs of degenerate size.

Every other whole-model test feeds doubled (symmetric) edges, where the packer
sets ``transpose_aliased`` and the kernels read ``col`` / ``p1`` for both
directions.  ``asymmetric`` builds batches whose node-level *and* pooled
adjacency are asymmetric; ``degenerate`` builds the smallest and the
tile-boundary graphs (N = 1, no edges, K0 = N, a hub row, N at and beside 16,
32, 64, 128).  Both return lists of ``oracle.pyg_ops.Data``.

For the VanillaNetwork pipeline (clusters dropped, any F and Fe):
``dense_tiles`` crosses the register budget of the chunk kernels' prologues
(a 64-row tile with more than 2,048 CSR edges, one with more than 2,048
transposed edges, a halo of more than 256 rows), ``hub`` makes one row wide
enough to overflow a workgroup's LDS carve, ``widths`` is a small asymmetric
batch at any feature widths, and ``between_small`` puts such a graph between
small ones so that none of its tiles' offsets is zero.
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


def without_clusters(datas):
    """The same graphs for a model that does not pool (VanillaNetwork)."""
    for d in datas:
        d.cluster0 = d.cluster1 = None
    return datas


def resized(datas, f, fe, seed=77):
    """``datas`` with ``f`` node-feature and ``fe`` edge-feature columns:
    leading columns kept, missing ones drawn (seeded) from N(0, 1) for x and
    N(0, 0.5) for the edge attributes; ``fe`` = 0 leaves an [E, 0] array."""
    rng = np.random.default_rng(seed)
    for d in datas:
        x, ea = d.x.numpy(), d.edge_attr.numpy().reshape(d.edge_index.shape[1], d.edge_attr.shape[-1])
        more_x = rng.normal(size=(x.shape[0], max(0, f - x.shape[1]))).astype(np.float32)
        more_ea = (0.5 * rng.normal(size=(ea.shape[0], max(0, fe - ea.shape[1])))).astype(np.float32)
        d.x = torch.from_numpy(np.ascontiguousarray(np.concatenate([x, more_x], axis=1)[:, :f]))
        d.edge_attr = torch.from_numpy(np.ascontiguousarray(np.concatenate([ea, more_ea], axis=1)[:, :fe]))
    return datas


def _plain(rng, x, ei, ea, name):
    d = P.Data(
        x=torch.from_numpy(x.astype(np.float32)),
        edge_index=torch.from_numpy(np.ascontiguousarray(ei, dtype=np.int64)).reshape(2, -1),
        edge_attr=torch.from_numpy(np.ascontiguousarray(ea, dtype=np.float32)).reshape(ei.shape[1], -1),
        y=torch.tensor([float(rng.uniform())]),
    )
    d.entry_names = name
    return d


DENSE_N, DENSE_DEG, DENSE_ISOLATED = 400, 40, 200
KPT_ITEMS = 2048  # items per workgroup that the chunk kernels' prologues keep in registers (vanilla_fused.hip: KPT * CT)


def tile_counts(d, tile_rows=64):
    """Per tile of ``tile_rows`` rows of the graph ``d``, from its edge list
    alone: (CSR edges ne, transposed edges nq, halo rows H = distinct out- and
    in-neighbours of the tile's rows)."""
    src, dst = d.edge_index.numpy()
    out = []
    for r0 in range(0, d.x.shape[0], tile_rows):
        o, i = (src >= r0) & (src < r0 + tile_rows), (dst >= r0) & (dst < r0 + tile_rows)
        out.append((int(o.sum()), int(i.sum()), int(np.union1d(dst[o], src[i]).size)))
    return out


def dense_tiles(fe, f=30):
    """One graph of 400 nodes, every edge stored once (asymmetric).  Rows 0-63
    have 40 out-edges each to distinct targets spread over the whole graph:
    tile 0 has ne = 2,560 CSR edges and a halo of more than 256 rows.  Rows
    64-127 each receive 40 edges from distinct sources among rows 128-399 and
    have two out-edges: tile 1 has nq > 2,048 transposed edges and ne < 2,048.
    Rows 128-399 have two more out-edges each among themselves, so the other
    tiles stay sparse.  Node 200 has no edge at all, node 150 a self loop, and
    the last edge of row 0 is stored twice.  Edge attributes: a distance in
    3-9, a 0/1 flag, then N(0, 0.5) columns (``fe`` of them kept)."""
    rng = np.random.default_rng(31)
    n, iso = DENSE_N, DENSE_ISOLATED
    ok = np.setdiff1d(np.arange(n), [iso])
    far = np.setdiff1d(np.arange(128, n), [iso])
    edges = []
    for i in range(64):
        edges += [(i, int(j)) for j in rng.choice(np.setdiff1d(ok, [i]), size=DENSE_DEG, replace=False)]
    for j in range(64, 128):
        edges += [(int(i), j) for i in rng.choice(far, size=DENSE_DEG, replace=False)]
        edges += [(j, int(k)) for k in rng.choice(np.setdiff1d(ok, [j]), size=2, replace=False)]
    for i in far:
        edges += [(int(i), int(k)) for k in rng.choice(np.setdiff1d(far, [i]), size=2, replace=False)]
    edges += [(150, 150), edges[DENSE_DEG - 1]]
    ei = np.asarray(edges, np.int64).T
    e = ei.shape[1]
    ea = np.concatenate([rng.uniform(3.0, 9.0, size=(e, 1)), rng.integers(0, 2, size=(e, 1)), 0.5 * rng.normal(size=(e, max(0, fe - 2)))], axis=1)[:, :fe]
    ea[-1] = ea[DENSE_DEG - 1]
    d = _plain(rng, rng.normal(size=(n, f)), ei, ea, "dense_tiles")
    (ne0, _, h0), (ne1, nq1, _), *rest = tile_counts(d)
    assert ne0 > KPT_ITEMS and h0 * 8 > KPT_ITEMS and nq1 > KPT_ITEMS and ne1 < KPT_ITEMS
    assert all(a < KPT_ITEMS and b < KPT_ITEMS for a, b, _ in rest)
    assert not (ei == iso).any() and len(set(edges)) == e - 1
    return d


HUB_TILED, HUB_UNTILED = 1000, 1200  # neighbours of the hub row; tests/test_vanilla_zoo_host.py places them with the host carves


def hub(n_neighbours, fe=3, f=30, y=None):
    """A graph of ``n_neighbours`` + 10 nodes whose node 3 has an out-edge to
    every node from 4 to ``n_neighbours`` + 3 and no edge back, plus 48 other
    directed edges that avoid node 3.  ``y``: its regression target (default:
    drawn like the other graphs')."""
    rng = np.random.default_rng(57)
    n = n_neighbours + 10
    others = np.setdiff1d(np.arange(n), [3])
    extra = np.stack([rng.choice(others, size=48), rng.choice(others, size=48)])
    ei = np.concatenate([np.stack([np.full(n_neighbours, 3), np.arange(4, n_neighbours + 4)]), extra], axis=1)
    e = ei.shape[1]
    ea = 0.5 * rng.normal(size=(e, fe))
    d = _plain(rng, 0.5 * rng.normal(size=(n, f)), ei, ea, f"hub{n_neighbours}")
    assert not (ei[1] == 3).any()
    if y is not None:
        d.y = torch.tensor([float(y)])
    return d


def between_small(d, fe=3, f=30):
    """[N = 1, a 65-node asymmetric graph, ``d``, N = 20 without edges]: a
    batch in which ``d`` has graphs, rows, edges and halo entries before it, so
    every offset of its tiles (``h0``, ``lcol_off``, ``ltcol_off``, ``word0``,
    and past its first tile ``e0``, ``q0``) is non-zero."""
    one, _, none, *_ = degenerate()
    (mid,) = asymmetric(1, seed=9, frac=0.6, n_lo=65, n_hi=65)
    small = without_clusters(resized([one, mid, none], f, fe))
    for s in small:
        del s.pos
    return [small[0], small[1], d, small[2]]


def widths(f, fe):
    """Three asymmetric graphs of 30-70 nodes and one of 130 (three 64-row
    chunks, two rows in the last), with ``f`` and ``fe`` feature columns."""
    datas = asymmetric(3, seed=12, frac=0.6) + asymmetric(1, seed=13, frac=0.6, n_lo=130, n_hi=130)
    return without_clusters(resized(datas, f, fe))


def batch(datas):
    """A fresh collated batch (the oracle's models modify theirs in place)."""
    return P.Batch.from_data_list([d.clone() for d in datas])
