"""Diagnostic: one graph pass (forward + backward partials) of GINet, FoutNet or
SGAT on seeded graphs, dumped to .npz, to compare two builds of the library bit
for bit with tools/cmp_dump.py (DR_LIB_NAME selects the build).

    DR_LIB_NAME=libdeeprank2_amd_<v>.so python tools/pass_dump.py <out.npz> [B] [n_lo n_hi]
        [--model ginet|foutnet|sgat] [--dtype f32|bf16] [--force-large]
        [--no-halos] [--no-atomic-max] [--tile ROWS] [--passes K]
    DR_LIB_NAME=... python tools/pass_dump.py <dir> --matrix

The large-path switches are BatchHandle's (force_large, large_halos,
large_atomic_max, large_tile).  Dumped: out, slab, head, loss_per_graph of the
last of K passes on the one handle (not plan.z, whose rows that are no pooling
arg candidate are uninitialised by design).
"""

from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "deeprank-gnn-2_amd")]

from bench import records  # noqa: E402
from deeprank2_amd import _lib  # noqa: E402
from deeprank2_amd.fused import BatchHandle, Dropout, make_pass, run_pass  # noqa: E402
from deeprank2_amd.neuralnets.gnn import foutnet, ginet, sgat  # noqa: E402
from deeprank2_amd.store import GraphStore, pack_graphs  # noqa: E402
from deeprank2_amd.utils.synthetic import make_dataset  # noqa: E402

MODELS = {"ginet": (ginet, ginet.GINet, 3), "foutnet": (foutnet, foutnet.FoutNet, 3), "sgat": (sgat, sgat.SGAT, 1)}  # module, class, edge features


def dump(path, B=64, fam=None, model="ginet", dtype="f32", force_large=False, halos=True, atomic_max=True, tile=None, passes=1):
    mod, cls, fe = MODELS[model]
    dev = torch.device("cuda:0")
    store = GraphStore(pack_graphs(records(make_dataset(B, seed=1000, **(fam or {})), edge_features=fe)), dev, dtype=dtype)
    h = BatchHandle(store, np.arange(B))
    h.force_large, h.large_halos, h.large_atomic_max, h.large_tile = force_large, halos, atomic_max, tile
    torch.manual_seed(0)
    params = cls(30, 1, fe).to(dev).ordered_params()
    fo = mod if model == "ginet" else foutnet  # SGAT shares FoutNet's partial layout
    for _ in range(passes):  # (zeros: what a pass leaves unwritten compares equal)
        out = torch.zeros(B, 1, device=dev)
        slab = torch.zeros(B * fo.slab_stride(30), device=dev)
        head = torch.zeros(B * fo.head_stride(1), device=dev)
        lpg = torch.zeros(B, device=dev)
        p = make_pass(1, 3, dropout=Dropout(0.4, seed=1, offset=0) if model == "ginet" else None, loss_kind=1, loss_scale=1 / B, out=out, loss_per_graph=lpg, slab=slab, head=head)
        p.compute_dtype = _lib.DR_DTYPE_BF16 if dtype == "bf16" else _lib.DR_DTYPE_F32
        run_pass(mod.SPEC, h, params, p)
        torch.cuda.synchronize()
    n = np.diff(store.packed.node_off)[:B]
    np.savez(path, out=out.cpu().numpy(), slab=slab.view(B, -1).cpu().numpy(), head=head.view(B, -1).cpu().numpy(), lpg=lpg.cpu().numpy())
    print("saved", path, "N range", (int(n.min()), int(n.max())), flush=True)


def matrix(outdir):
    """The large path's switches crossed: 8 residue graphs forced through it, two
    passes per handle, and per model 2 atom-level graphs on their natural path."""
    os.makedirs(outdir, exist_ok=True)
    for model, dtype in (("ginet", "f32"), ("ginet", "bf16"), ("foutnet", "f32"), ("sgat", "f32")):
        for halos in (True, False):
            for amax in (True, False) if model == "ginet" else (True,):
                for tile in (16, 64, 128):
                    name = f"{model}_{dtype}_halos{int(halos)}_amax{int(amax)}_tile{tile}.npz"
                    dump(os.path.join(outdir, name), 8, None, model, dtype, True, halos, amax, tile, passes=2)
        dump(os.path.join(outdir, f"{model}_{dtype}_atom.npz"), 2, {"n_lo": 2700, "n_hi": 3300}, model, dtype)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("path", help="the .npz to write (with --matrix: the directory)")
    ap.add_argument("B", type=int, nargs="?", default=64)
    ap.add_argument("n_lo", type=int, nargs="?")
    ap.add_argument("n_hi", type=int, nargs="?")
    ap.add_argument("--model", choices=list(MODELS), default="ginet")
    ap.add_argument("--dtype", choices=["f32", "bf16"], default="f32")
    ap.add_argument("--force-large", action="store_true")
    ap.add_argument("--no-halos", action="store_true")
    ap.add_argument("--no-atomic-max", action="store_true")
    ap.add_argument("--tile", type=int, default=None)
    ap.add_argument("--passes", type=int, default=1)
    ap.add_argument("--matrix", action="store_true", help="dump every combination of the large path's switches into the directory `path`")
    a = ap.parse_args()
    if a.matrix:
        matrix(a.path)
        return
    fam = {"n_lo": a.n_lo, "n_hi": a.n_hi} if a.n_hi is not None else None
    dump(a.path, a.B, fam, a.model, a.dtype, a.force_large, not a.no_halos, not a.no_atomic_max, a.tile, a.passes)


if __name__ == "__main__":
    main()
