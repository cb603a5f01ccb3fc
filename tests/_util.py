"""Helpers shared by the test modules (golden arrays -> inputs, state dicts)."""

from __future__ import annotations

import atexit
import gzip
import json
import os
import shutil
import tempfile

import numpy as np
import torch

from oracle import pyg_ops as P


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_h5_dir = None
_pretrained = None


def golden_hdf5_dir():
    """DeepRank2's own test files (``tests/golden/hdf5/*.hdf5.gz``, stored by
    ``tests/golden/make_hdf5_fixtures.py``) unpacked once per process into a
    temporary directory; returns that directory."""
    global _h5_dir  # noqa: PLW0603
    if _h5_dir is None:
        d = tempfile.mkdtemp(prefix="golden_hdf5_")
        atexit.register(shutil.rmtree, d, ignore_errors=True)
        src = os.path.join(GOLDEN, "hdf5")
        for name in sorted(os.listdir(src)):
            if name.endswith(".hdf5.gz"):
                with gzip.open(os.path.join(src, name), "rb") as f, open(os.path.join(d, name[: -len(".gz")]), "wb") as g:
                    shutil.copyfileobj(f, g)
        _h5_dir = d
    return _h5_dir


def golden_pretrained():
    """DeepRank2's pre-trained VanillaNetwork checkpoint, written once per
    process in the reference's format (``Trainer._save_model``: ``torch.save``
    with dill) from its stored data (``tests/golden/pretrained``: tensors in
    the ``.npz``, everything else in the ``.json``); returns the file's path.

    As in the reference's file, live objects stand beside the data: the
    dataset class and the optimizer's class pickled by value (dill's
    ``_create_type``; the classes here are local stand-ins of the same names),
    an optimizer instance carrying the stored state, a loss-function instance,
    and numpy scalars for the means / devs — so ``torch.load(weights_only=True)``
    refuses the file and ``io.checkpoint``'s opcode reader has to read it."""
    global _pretrained  # noqa: PLW0603
    if _pretrained is not None:
        return _pretrained
    import dill  # noqa: PLC0415

    stem = os.path.join(GOLDEN, "pretrained", "testing_graph_model")
    with open(stem + ".json") as f:
        state = json.load(f)
    with np.load(stem + ".npz", allow_pickle=False) as z:
        tensors = {k: torch.from_numpy(z[k]) for k in z.files}
    model_state = {k.split("/", 1)[1]: v for k, v in tensors.items() if k.startswith("model_state/")}
    opt_state = {}
    for k, v in tensors.items():
        if k.startswith("optimizer_state/"):
            _, i, name = k.split("/")
            opt_state.setdefault(int(i), {})[name] = v
    groups = state.pop("param_groups")
    for g in groups:
        g["betas"] = tuple(g["betas"])
    state["classes_to_index"] = {k: v for k, v in state["classes_to_index"]}
    state["means"] = {k: np.float64(v) for k, v in state["means"].items()}
    state["devs"] = {k: np.float64(v) for k, v in state["devs"].items()}
    # classes of module __main__ that no module holds: dill pickles them by value
    adam = type(state["optimizer"], (torch.optim.Adam,), {"__module__": "__main__"})
    assert state["lossfunction"] == "CrossEntropyLoss"
    optimizer = adam([torch.nn.Parameter(v.clone()) for v in model_state.values()], lr=state["lr"], weight_decay=state["weight_decay"])
    optimizer.load_state_dict({"state": opt_state, "param_groups": groups})
    state.update(
        data_type=type(state["data_type"], (), {"__module__": "__main__"}),
        model_state=model_state,
        optimizer=optimizer,
        optimizer_state={"state": opt_state, "param_groups": groups},
        lossfunction=torch.nn.CrossEntropyLoss(),
    )
    d = tempfile.mkdtemp(prefix="golden_pretrained_")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    path = os.path.join(d, "testing_graph_model.pth.tar")
    torch.save(state, path, pickle_module=dill)
    _pretrained = path
    return path


def golden_batch(z):
    """Rebuild the collated PyG-style batch stored by tests/golden/make_golden.py."""
    b = P.Batch()
    for k in ("x", "edge_index", "edge_attr", "batch", "cluster0", "cluster1", "y", "pos", "ptr"):
        key = "in/" + k
        if key in z:
            arr = z[key]
            t = torch.from_numpy(np.array(arr))
            b.__dict__[k] = t
    return b


def golden_state_dict(z):
    return {k[len("param/"):]: torch.from_numpy(np.array(v)) for k, v in z.items() if k.startswith("param/")}


def golden_grads(z):
    return {k[len("grad/"):]: np.array(v) for k, v in z.items() if k.startswith("grad/")}


def fixed_dropout(mask):
    def _drop(x, p, training):
        return x * mask / (1.0 - p) if training else x

    return _drop


def assert_grad_close(actual, ref, rtol=1e-4, ntol=1e-6, err_msg=""):
    """Gradient parity: elementwise rtol plus a normwise floor ntol*max|ref|.

    fp32 reassociation (the MI355X path aggregates A·X before the GEMM; the
    reference multiplies per edge, then scatter-adds) leaves absolute errors
    that scale with the tensor's largest entries (~1e3 on the 1ATN fixture),
    so tiny entries of a large gradient need the normwise floor."""
    ref = np.asarray(ref)
    fin = np.abs(ref[np.isfinite(ref)])
    scale = float(fin.max()) if fin.size else 0.0  # NaN entries must match NaN (assert_allclose equal_nan)
    np.testing.assert_allclose(np.asarray(actual), ref, rtol=rtol, atol=max(1e-6, ntol * scale), err_msg=err_msg)


def golden_graphs(z):
    """Per-graph (local edge_index, num_nodes, cluster0, cluster1) of a stored
    collated batch (``in/ptr`` node offsets; cluster1 has one entry per
    depth-0 cluster of each graph)."""
    ptr, ei, c0, c1 = (np.asarray(z[f"in/{k}"]) for k in ("ptr", "edge_index", "cluster0", "cluster1"))
    out, k1 = [], 0
    for g in range(ptr.size - 1):
        lo, hi = int(ptr[g]), int(ptr[g + 1])
        m = (ei[0] >= lo) & (ei[0] < hi)
        a = c0[lo:hi]
        k = int(a.max()) + 1 if a.size else 0
        out.append((ei[:, m] - lo, hi - lo, a, c1[k1 : k1 + k]))
        k1 += k
    assert k1 == c1.size
    return out


def dwc_mask(n_slab, n_graphs, fe, F=30):
    """Slab positions of dWc (the edge-attribute columns of both layers' edge
    MLP weight) in graph rows 0..n_graphs-1 of an n_slab-float slab: tiles that
    divide the 64-row weight-gradient chunks sum them per tile first, another
    fp32 order than the per-row path."""
    KE = 2 * F + fe
    LG = 32 * KE + 32 + F * (F + 32) + F
    wc = np.zeros(n_slab, bool)
    for b in range(n_graphs):
        for lay in range(2):
            for c in range(32):
                o = b * 2 * LG + lay * LG + c * KE + 2 * F
                wc[o : o + fe] = True
    return torch.from_numpy(wc)


def assert_same(res, wc=None):
    """Every tensor bit for bit, except the slab's dWc entries (wc) at 1e-5 of their scale."""
    import itertools

    for k, (a, b) in enumerate(itertools.zip_longest(*res)):
        if k == 1 and wc is not None:
            assert torch.equal(a[~wc], b[~wc])
            np.testing.assert_allclose(a[wc].numpy(), b[wc].numpy(), rtol=0, atol=1e-5 * float(b[wc].abs().max()))
        else:
            assert torch.equal(a, b)
