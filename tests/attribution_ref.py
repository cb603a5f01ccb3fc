"""TEST INFRASTRUCTURE: the CPU reference of the GINet input gradients.

The reference is the oracle model (``oracle/gnn_ref.GINet``) in eval mode with
``bat.x.requires_grad_()`` and ``torch.autograd.grad((out * seed).sum(), bat.x)``.

One thing stands between that sentence and a correct number.  GINet runs its
second branch on ``twin = data.clone()`` (ginet.py:92).  PyG's ``Data.clone``
clones tensor by tensor, which autograd follows back to ``x``; the oracle's
``Data.clone`` is a ``copy.deepcopy``, which makes the twin's ``x`` a new leaf,
so the ``conv1_ext`` branch's gradient never reaches ``bat.x`` (the outputs
are unaffected).  ``GradBatch`` restores PyG's behaviour for the batch handed
to the oracle; ``tests/test_attribution_host.py`` checks the result against
central differences of the oracle's own forward.
"""

from __future__ import annotations

import copy

import numpy as np
import torch

import graph_zoo
from oracle import pyg_ops as P


class GradBatch(P.Batch):
    def clone(self):
        new = copy.copy(self)
        new.__dict__ = {k: (v.clone() if isinstance(v, torch.Tensor) else copy.deepcopy(v)) for k, v in self.__dict__.items()}
        return new


def grad_batch(datas):
    bat = graph_zoo.batch(datas)
    bat.__class__ = GradBatch
    return bat


def seed_for(out, target, n, out_dim):
    """The upstream gradient ``input_gradients`` documents for ``target``
    (None, an index, "pred", or a [n, out_dim] tensor used as it is)."""
    if isinstance(target, torch.Tensor):
        return target.clone()
    seed = torch.zeros(n, out_dim)
    if isinstance(target, str):
        assert target == "pred"
        seed.scatter_(1, out.detach().argmax(dim=1, keepdim=True), 1.0)
    else:
        seed[:, 0 if target is None else int(target)] = 1.0
    return seed


def oracle_input_grad(model_o, datas, target):
    """(out [n, out_dim], dx [rows, F], seed [n, out_dim], node_off [n + 1]) as
    numpy arrays, from the eval-mode oracle ``model_o`` on the graphs ``datas``."""
    assert not model_o.training
    bat = grad_batch(datas)
    x = bat.x
    x.requires_grad_()
    out = model_o(bat)
    seed = seed_for(out, target, out.shape[0], out.shape[1])
    (g,) = torch.autograd.grad((out * seed).sum(), x)
    node_off = np.concatenate([[0], np.cumsum([d.x.shape[0] for d in datas])]).astype(np.int64)
    return out.detach().numpy(), g.numpy(), seed.numpy(), node_off
