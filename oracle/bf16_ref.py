"""TEST INFRASTRUCTURE ONLY (see ``oracle/__init__.py``).

GINet with the rounding points of the bf16 compute mode
(``ginet_large_conv1_bf16_kernel`` in ``csrc/ginet_fused.hip``), written from
the kernel's documented arithmetic, not fitted to its outputs:

1. ``xq = bf16(x)``: the store's bf16 copy of x (``GraphStore(dtype="bf16")``).
2. ``Z = bf16(A xq)`` per node: the row's neighbours are added one after the
   other in fp32, from 0, in stable-CSR order (the kernel's ``f4add`` chain),
   and the sum is rounded once.  Z is the GEMM operand *and* the workspace the
   tail reads for dW1, so the weight gradient consumes the rounded Z.
3. ``Wq = bf16(W)`` for ``conv1.fc.weight`` and ``conv1_ext.fc.weight``; the
   gradient passes straight through to the fp32 master weight.

``H = Z Wq^T`` is accumulated in fp32 (bf16 x bf16 products are exact in
fp32), so beyond these three points only the fp32 summation order of the GEMM
differs from the kernel.  The attention factor is identically 1 for finite
inputs (``gnn_ref.GINetConvLayer``): conv1 is restructured from
``scatter(fc(x[dst]))`` into ``(A x) W^T`` and conv1's ``fc_attention`` /
``fc_edge_attr`` receive no gradient (``.grad`` stays None; the kernel writes
exact zeros).  Everything after conv1 is ``gnn_ref.GINet`` unchanged.

The three quantisers are swappable callables (fp32 tensor -> fp32 tensor), so
tests can put the identity or truncation in their place.
"""

from __future__ import annotations

import numpy as np
import torch
from torch.nn import functional as tf

from oracle import gnn_ref
from oracle import pyg_ops as P


def bf16_rne(t: torch.Tensor) -> torch.Tensor:
    """Round to nearest even to bf16, returned as fp32 (the kernel's ``f2bf``)."""
    return t.to(torch.bfloat16).to(torch.float32)


def bf16_trunc(t: torch.Tensor) -> torch.Tensor:
    """Truncation to bf16 (the low 16 bits dropped): a *wrong* rounding, for sensitivity tests."""
    return (t.detach().contiguous().view(torch.int32) & -65536).view(torch.float32)


def identity(t: torch.Tensor) -> torch.Tensor:
    return t


def f2bf_bits(f: np.ndarray) -> np.ndarray:
    """The kernel's ``f2bf`` restated in numpy: fp32 array -> bf16 bit patterns
    (uint16).  ``u += 0x7fff + ((u >> 16) & 1)``; NaN -> quiet NaN."""
    u = np.ascontiguousarray(f, dtype=np.float32).view(np.uint32)
    nan = (u & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)
    r = (u.astype(np.uint64) + 0x7FFF + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint64(16)
    return np.where(nan, (u >> np.uint32(16)) | np.uint32(0x40), r).astype(np.uint16)


def stable_csr(edge_index: torch.Tensor, n: int):
    """CSR by ``edge_index[0]`` (the scatter index), stable: ``rowptr`` [n + 1],
    ``col`` [E] = ``edge_index[1]`` in that order.  Duplicate edges and self
    loops stay, each in its place."""
    rows = edge_index[0]
    order = torch.argsort(rows, stable=True)
    rowptr = torch.zeros(n + 1, dtype=torch.long)
    rowptr[1:] = torch.cumsum(torch.bincount(rows, minlength=n), 0)
    return rowptr, edge_index[1][order]


def sequential_row_sum(x: torch.Tensor, rowptr: torch.Tensor, col: torch.Tensor) -> torch.Tensor:
    """``out[i] = ((0 + x[col[e0]]) + x[col[e0 + 1]]) + ...`` in fp32, one
    neighbour slot at a time over all rows (each step is one IEEE fp32 add per
    element, so the result is that of the per-row loop, bit for bit)."""
    n = rowptr.numel() - 1
    deg = rowptr[1:] - rowptr[:-1]
    out = torch.zeros(n, x.shape[1], dtype=torch.float32)
    for s in range(int(deg.max()) if n else 0):
        rows = torch.nonzero(deg > s).reshape(-1)
        out[rows] = out[rows] + x[col[rowptr[rows] + s]]
    return out


class GINetBf16(gnn_ref.GINet):
    """``gnn_ref.GINet`` with the bf16 mode's conv1 (module docstring).
    Parameter names and shapes are those of ``gnn_ref.GINet``.

    After a forward, ``trace`` holds what the tests look at: ``z`` (the
    quantised Z, [N, F]), and per branch (conv, conv_ext) in ``h1`` / ``h2``
    the pre-ReLU conv1 / conv2 outputs, in ``pool0`` (relu(h1), dense depth-0
    cluster id per node), in ``pool1`` (relu(h2), dense depth-1 cluster id per
    pooled node) and in ``batch0`` / ``batch1`` the graph of each node / pooled
    node."""

    def __init__(self, input_shape, output_shape=1, input_shape_edge=1, quant_x=bf16_rne, quant_z=bf16_rne, quant_w=bf16_rne):
        super().__init__(input_shape, output_shape, input_shape_edge)
        self.quant_x, self.quant_z, self.quant_w = quant_x, quant_z, quant_w
        self.trace = None

    def _z(self, data):
        with torch.no_grad():
            rowptr, col = stable_csr(data.edge_index, data.x.shape[0])
            return self.quant_z(sequential_row_sum(self.quant_x(data.x), rowptr, col))

    def _branch(self, data, conv_a, conv_b, z):
        w = conv_a.fc.weight
        wq = w + (self.quant_w(w.detach()) - w.detach())  # value: rounded; gradient: straight to w
        h1 = z @ wq.t()
        data.x = tf.relu(h1)
        batch0 = data.batch
        c0, _ = P.consecutive_cluster(gnn_ref.offset_clusters_inplace(data.cluster0, data.batch))
        pool0 = (data.x.detach(), c0)
        data = gnn_ref.pool_communities(data.cluster0, data)
        h2 = conv_b(data.x, data.edge_index, data.edge_attr)
        data.x = tf.relu(h2)
        c1 = gnn_ref.offset_clusters_inplace(data.cluster1, data.batch)
        d1, _ = P.consecutive_cluster(c1)
        for k, v in (("h1", h1.detach()), ("h2", h2.detach()), ("pool0", pool0), ("pool1", (data.x.detach(), d1)), ("batch0", batch0), ("batch1", data.batch)):
            self.trace[k].append(v)
        return P.max_pool_x(c1, data.x, data.batch)

    def forward(self, data):
        twin = data.clone()
        z = self._z(data)
        self.trace = {"z": z, "h1": [], "h2": [], "pool0": [], "pool1": [], "batch0": [], "batch1": []}
        x, b = self._branch(data, self.conv1, self.conv2, z)
        x_ext, b_ext = self._branch(twin, self.conv1_ext, self.conv2_ext, z)
        h = torch.cat([P.scatter_mean(x, b, dim=0), P.scatter_mean(x_ext, b_ext, dim=0)], dim=1)
        h = tf.relu(self.fc1(h))
        h = self.dropout_fn(h, self.dropout, training=self.training)
        return self.fc2(h)
