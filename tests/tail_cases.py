"""TEST INFRASTRUCTURE shared by ``test_tail_cases_host.py`` (CPU) and
``test_gpu_ginet_tail.py`` (GPU): GINet on graphs built from designed clusters,
so that the pooled graph the kernels' tail (``ginet_tail``: conv2 on the pooled
graph, the depth-1 pooling and its backward, dW2 / dP1, dW1) works on is
exactly what the case names, with one fp64 training step of the oracle
(``oracle/gnn_ref.py``) per case as the reference.

A case is a batch of two graphs (N <= 48) with the same pooled design and
different members per cluster.  Cluster c has ``1 + (c + g) % 3`` nodes chained
by undirected edges; a pooled edge (a, b) is one node-level edge between a
member of a and a member of b, undirected unless the case is directed.  The
tail's loops go in groups (2 neighbours in conv2 forward, 4 in the pooling
backward, 4 members of the one depth-1 cluster in its tie count) and end with
a group of exactly the remaining size, so the designs put a row's degree at,
below and above each group size and its multiples, and K0 on both sides of
every switch in the tail (12: direct loops | MFMA for dW2 and
dP1; 16: one-cluster | general pooling).

Dropout: the kernels' own hash (``DR_DROPOUT_HASH``, seed ``DROP_SEED``, step
counter 0); the oracle is fed the host replica of the same keep flags.
Loss: MSE on targets ``Y_BASE + g`` for OUT = 1, cross entropy with targets
``g % 2`` for OUT = 2.
"""

from __future__ import annotations

import functools
import itertools

import numpy as np
import torch
from _util import fixed_dropout

import graph_zoo
from oracle import gnn_ref

DROP_SEED = 4242
DROP_P = 0.4
WIDTHS = (8, 30)
N_MAX = 48
GRAPHS = 2
# Node features N(0, 1) * X_SCALE drawn per design under SEED, weights under
# W_SEED, MSE targets Y_BASE + g (away from the outputs, so the loss gradient is
# no cancellation).  The fp32 oracle's own distance from the fp64 one depends on
# these draws (0.08 to 0.6 of the tolerance over 100 draws tried: small gradient
# elements are sums of cancelling terms, held to 1e-6 of the tensor's largest)
# and, a little, on the CPU's BLAS path; these values keep every case within a
# tenth on both kinds of machine the suite runs on (0.088 and 0.081,
# test_tail_cases_host.py).
X_SCALE = 0.25
SEED = 84
W_SEED = 13
Y_BASE = 3.0


def _complete(k):
    return tuple(itertools.combinations(range(k), 2))


def _path(k):
    return tuple((i, i + 1) for i in range(k - 1))


# name -> (K0, depth-1 cluster of each depth-0 cluster, undirected pooled pairs, directed pooled edges)
DESIGNS = {
    "k1_no_edge": (1, (0,), (), ()),
    "k5_path": (5, (0,) * 5, _path(5), ()),
    "k5_complete": (5, (0,) * 5, _complete(5), ()),
    "k6_complete": (6, (0,) * 6, _complete(6), ()),
    "k9_complete": (9, (0,) * 9, _complete(9), ()),
    "k10_complete": (10, (0,) * 10, _complete(10), ()),
    "k11_complete": (11, (0,) * 11, _complete(11), ()),
    "k12_complete": (12, (0,) * 12, _complete(12), ()),
    "k15_complete": (15, (0,) * 15, _complete(15), ()),
    "k16_complete": (16, (0,) * 16, _complete(16), ()),
    "k17_complete": (17, (0,) * 17, _complete(17), ()),
    "k9_star": (9, (0,) * 9, tuple((0, i) for i in range(1, 9)), ()),
    "k5_isolated": (5, (0,) * 5, ((0, 1), (1, 3), (3, 4), (0, 4)), ()),
    # 0 -> 1, 2, 3, 4 and 1 -> 2, 3 -> 1, 4 -> 0: rows of degree 4, 1, 0, 1, 1, transposed rows of 1, 2, 2, 1, 1
    "k5_directed": (5, (0,) * 5, (), ((0, 1), (0, 2), (0, 3), (0, 4), (1, 2), (3, 1), (4, 0))),
    "k6_two_depth1": (6, (0, 0, 0, 1, 1, 1), _complete(6), ()),
    "k6_three_depth1_singleton": (6, (0, 0, 0, 1, 1, 2), _complete(6), ()),
}
CE_CASES = ("k5_complete", "k12_complete", "k6_three_depth1_singleton")


def all_cases():
    """(name, F, OUT) of every case: MSE on all designs, two-class CE on three."""
    return [(n, f, 1) for n in DESIGNS for f in WIDTHS] + [(n, f, 2) for n in CE_CASES for f in WIDTHS]


def case_id(c):
    return f"{c[0]}-F{c[1]}-OUT{c[2]}"


def pooled_rows(name):
    """The design's pooled CSR rows and transposed rows (sorted neighbour
    lists per cluster), as the packer must produce them."""
    k0, _, pairs, directed = DESIGNS[name]
    edges = set(pairs) | {(b, a) for a, b in pairs} | set(directed)
    rows = [sorted(c for r, c in edges if r == k) for k in range(k0)]
    trows = [sorted(r for r, c in edges if c == k) for k in range(k0)]
    return rows, trows


def _design_graph(name, g):
    k0, c1, pairs, directed = DESIGNS[name]
    size = [1 + (c + g) % 3 for c in range(k0)]
    first = np.concatenate([[0], np.cumsum(size)])
    n = int(first[-1])
    assert n <= N_MAX
    cluster0 = np.repeat(np.arange(k0), size)
    inner = [(int(first[c]) + i, int(first[c]) + i + 1) for c in range(k0) for i in range(size[c] - 1)]

    def node(a, b):  # the member of a that carries its edge to b
        return int(first[a]) + b % size[a]

    und = inner + [(node(a, b), node(b, a)) for a, b in pairs]
    one = [(node(a, b), node(b, a)) for a, b in directed]
    rng = np.random.default_rng(SEED * (sorted(DESIGNS).index(name) + 1) + g)
    return graph_zoo._graph(rng, n, und, cluster0, c1, f"{name}{g}", directed=one)  # noqa: SLF001


def datas(name, f, out):
    """The two graphs of one case, built once per process and left unchanged
    (collate copies of them with ``graph_zoo.batch``)."""
    return _datas(name, f, out)


@functools.lru_cache(maxsize=None)
def _datas(name, f, out):
    ds = graph_zoo.resized([_design_graph(name, g) for g in range(GRAPHS)], f, 3)
    for d in ds:
        d.x = d.x * X_SCALE
    for g, d in enumerate(ds):
        d.y = torch.tensor([float(g % out) if out > 1 else Y_BASE + g])
    return tuple(ds)


@functools.lru_cache(maxsize=None)
def packed(name, f, out):
    """The case's graphs in the store layout (host side; shared, unchanged)."""
    from deeprank2_amd.store import pack_graphs, records_from_batch  # noqa: PLC0415

    return pack_graphs(records_from_batch(graph_zoo.batch(datas(name, f, out))))


@functools.lru_cache(maxsize=None)
def keep_mask():
    """The keep flags the kernels' hash draws for the first step of a batch of
    ``GRAPHS`` graphs (host replica), as float [GRAPHS, 128]."""
    from deeprank2_amd import _lib  # noqa: PLC0415

    return torch.from_numpy(_lib.dropout_keep_host(DROP_SEED, 0, GRAPHS * 128, DROP_P).reshape(GRAPHS, 128).astype(np.float32))


def oracle(name, f, out, dtype=torch.float64):
    """One training-mode forward + backward of the oracle in ``dtype``:
    ``{"state", "out", "loss", "grads"}``; the weights are drawn in fp32 under
    seed ``W_SEED`` (``state``: what the HIP model loads).  Cached per case and dtype."""
    return _oracle(name, f, out, dtype)


@functools.lru_cache(maxsize=None)
def _oracle(name, f, out, dtype):
    ds = datas(name, f, out)
    assert torch.get_default_dtype() == torch.float32
    torch.manual_seed(W_SEED)
    model = gnn_ref.GINet(f, out, 3).train()
    assert model.dropout == DROP_P
    state = {k: v.detach().clone() for k, v in model.state_dict().items()}
    model.dropout_fn = fixed_dropout(keep_mask().to(dtype))
    model = model.to(dtype)
    torch.set_default_dtype(dtype)  # oracle/pyg_ops.py and the layers allocate in the default dtype
    try:
        bat = graph_zoo.batch(ds)
        for k in ("x", "edge_attr", "pos", "y"):
            setattr(bat, k, getattr(bat, k).to(dtype))
        y = bat.y.clone()
        res = model(bat)
        lval = torch.nn.functional.mse_loss(res.reshape(-1), y) if out == 1 else torch.nn.functional.cross_entropy(res, y.long())
        lval.backward()
    finally:
        torch.set_default_dtype(torch.float32)
    grads = {n: p.grad.detach().numpy().copy() for n, p in model.named_parameters()}
    return {"state": state, "out": res.detach().numpy().copy(), "loss": float(lval.detach()), "grads": grads}
