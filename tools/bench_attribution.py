"""Measurement: GINet input gradients (``attribution.input_gradients``), the
fused pass against what the parent commit offers for the same numbers.

configs[1]-shape synthetic graphs, one batch of B = 64.

Through the public call, from the first host instruction to the device idle:

* ``api_fused``      ``input_gradients(model, store, batch)``: one
                     ``dr_ginet_input_grad_pass`` launch;
* ``api_layers``     ``input_gradients(..., fused=False)``: ``layered.ginet_forward``
                     with ``x`` requiring grad, then ``torch.autograd.grad`` — the
                     only route to these numbers at the parent: the baseline.

With everything a caller can keep between batches kept (the handle, the batch
tensors and their pooling plan, the buffers):

* ``launch_ig``      the bare ``dr_ginet_input_grad_pass`` launch;
* ``launch_pass_z``  ``dr_ginet_graph_pass_z`` with FORWARD | BACKWARD on the same
                     batch: the difference prices the epilogue (dZ, dX = A^T dZ);
* ``layers_steady``  the layer route's forward + ``autograd.grad`` alone.

Wall-clock us per batch (``--reps`` calls per timing, the device idle before
and after).  The variants are interleaved in one process and each runs
``--runs`` times; the table gives the mean and the spread (max - min).  The
last lines say whether the fused route beats the layer route by more than five
times that route's own spread (the bar for keeping it the default).

``--large`` measures the tile route on atom-level graphs instead
(``main_large``: the public call with ``tiles=True`` against the layer route,
the parent's only route for these graphs, and the bare passes), by the same
rules.

``--ig`` measures integrated gradients instead (``main_ig``: the bare
``dr_ginet_integrated_grad_pass`` for each group count, the public call, and
the layer route as the baseline), by the same rules.

``--ig --large`` measures integrated gradients on the tile route
(``main_ig_large``: the bare ``dr_ginet_large_integrated_grad_pass`` for each
group count, the public call with ``tiles=True``, and the layer route as the
baseline) on the ``--large`` batch.
"""

from __future__ import annotations

import argparse
import copy
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "deeprank-gnn-2_amd")]

from bench import make_graphs, records  # noqa: E402
from deeprank2_amd import _lib, attribution, layered  # noqa: E402
from deeprank2_amd.fused import BatchHandle, make_pass, z_lds_for  # noqa: E402
from deeprank2_amd.neuralnets.gnn import ginet  # noqa: E402
from deeprank2_amd.store import GraphStore, pack_graphs  # noqa: E402

B = 64


def wall_us(body, reps):
    """us per call of ``reps`` calls of ``body``, the device idle before and after."""
    body()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        body()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / reps


def interleaved(variants, runs, reps):
    times = {name: [] for name in variants}
    for _ in range(runs):
        for name, body in variants.items():
            times[name].append(wall_us(body, reps))
    return times


IG_STEPS = 32
IG_GROUPS = (1, 2, 4, 8, 32)


def main_ig(args):
    """``--ig``: integrated gradients, 32 Gauss-Legendre nodes, zero baseline.

    * ``pass_gG``        the bare ``dr_ginet_integrated_grad_pass`` (both launches)
                         with G workgroups per graph, G in 1, 2, 4, 8, 32;
    * ``pass_mean``      the same at the default G with a per-feature mean
                         baseline: the difference prices the Zb reads;
    * ``api_fused``      ``integrated_gradients(model, store, batch)``;
    * ``api_layers``     ``integrated_gradients(..., fused=False)``: 32 times the
                         layer forward + ``autograd.grad``, the only route the
                         parent offers: the baseline."""
    dev = torch.device("cuda:0")
    store = GraphStore(pack_graphs(records(make_graphs("residue", B, 1000))), dev)
    torch.manual_seed(0)
    model = ginet.GINet(30, 1, 3).to(dev).eval()
    idx = np.arange(B)
    f, xs, out_dim = store.n_feat, store.x_stride, 1

    def api_fused():
        return attribution.integrated_gradients(model, store, indices=idx, batch_size=B, steps=IG_STEPS, fused=True)

    def api_layers():
        return attribution.integrated_gradients(model, store, indices=idx, batch_size=B, steps=IG_STEPS, fused=False)

    a, b = api_fused(), api_layers()
    assert a.path == "fused" and b.path == "layers"
    scale = float(b.attr.abs().max())
    assert torch.allclose(a.attr, b.attr, rtol=1e-4, atol=max(1e-6, 1e-6 * scale)) and torch.allclose(a.out, b.out, rtol=1e-4, atol=1e-4), "the two routes agree"
    print(f"completeness: max |delta| {float(a.delta.abs().max()):.3e} against a mean sum|attr| of {float(a.attr.abs().sum()) / B:.3e} per graph")

    h = BatchHandle(store, idx.astype(np.int32))
    params = [p.detach().contiguous() for p in model.ordered_params()]
    w = ginet.weights_c(params)
    z, zs = store.agg_x(), store.agg_x_stride
    lib = _lib.load()
    stream = _lib.stream_ptr(dev)
    seed = torch.ones(B, out_dim, device=dev)
    p = make_pass(out_dim, _lib.DR_PASS_FORWARD | _lib.DR_PASS_BACKWARD, dout=seed)
    rows = int(a.node_off[-1])
    attr = torch.empty(rows, xs, device=dev)
    off = torch.from_numpy(a.node_off[:-1].copy()).to(dev)
    alpha, weight = torch.from_numpy(a.alpha).to(dev), torch.from_numpy(a.weight).to(dev)
    attr_sum = torch.empty(B, dtype=torch.float64, device=dev)
    alias = int(store.packed.transpose_aliased)
    lds = int(lib.dr_ginet_integrated_grad_lds_bytes(*h.max_sizes[:2], f, *h.max_sizes[2:], alias, out_dim, zs))
    gmax = max(IG_GROUPS)
    slab = torch.empty(gmax * B * ginet.slab_stride(f), device=dev)
    head = torch.zeros(gmax * B * ginet.head_stride(out_dim), device=dev)
    outs = torch.empty(gmax * B * out_dim, device=dev)
    part = torch.empty(gmax, rows, xs, device=dev)
    # the mean baseline in x's layout and its neighbour sums
    xb = torch.zeros_like(store.x)
    xb[:, :f] = store.x[:, :f].mean(dim=0)
    zb = torch.empty_like(z)
    st = _lib.GraphStoreC.from_buffer_copy(store.cstruct())
    st.x = xb.data_ptr()
    _lib.check(lib.dr_aggregate_x(st, zb.data_ptr(), zs, 0, store.n_graphs, stream), "dr_aggregate_x")

    def bare(groups, baseline=False):
        ig = _lib.IntegratedGradC()
        ig.attr, ig.row_off, ig.dx_stride = attr.data_ptr(), off.data_ptr(), xs
        ig.n_steps, ig.n_groups = IG_STEPS, groups
        ig.alpha, ig.weight = alpha.data_ptr(), weight.data_ptr()
        ig.zb, ig.xb = (zb.data_ptr(), xb.data_ptr()) if baseline else (None, None)
        ig.part, ig.part_off, ig.part_rows = part.data_ptr(), off.data_ptr(), rows
        ig.attr_sum = attr_sum.data_ptr()
        ig.slab, ig.head, ig.out = slab.data_ptr(), head.data_ptr(), outs.data_ptr()

        def body():
            _lib.check(lib.dr_ginet_integrated_grad_pass(store.cstruct(), h.descs.data_ptr(), B, w, p, ig, z.data_ptr(), zs, lds, stream), "dr_ginet_integrated_grad_pass")

        return body

    gdef = min(attribution.IG_GROUPS_DEFAULT, IG_STEPS)
    bare(gdef)()
    torch.cuda.synchronize()
    assert torch.equal(attr[:, :f], a.attr), "the bare launch writes the public call's bits"

    variants = {f"pass_g{g}": bare(g) for g in IG_GROUPS}
    variants["pass_mean"] = bare(gdef, baseline=True)
    variants["api_fused"] = api_fused
    variants["api_layers"] = api_layers
    times = interleaved(variants, args.runs, args.reps)
    rows_j = []
    print(f"{'variant':>12} {'us/batch':>10} {'spread us':>10}  runs")
    for name, ts in times.items():
        mean, spread = float(np.mean(ts)), float(max(ts) - min(ts))
        rows_j.append({"variant": name, "us": round(mean, 2), "spread_us": round(spread, 2), "runs_us": [round(x, 2) for x in ts]})
        print(f"{name:>12} {mean:10.1f} {spread:10.1f}  {' '.join(f'{x:.1f}' for x in ts)}")
    best = min(IG_GROUPS, key=lambda g: np.mean(times[f"pass_g{g}"]))
    print(f"fastest groups: {best} (the default is {attribution.IG_GROUPS_DEFAULT})")
    step_us = float(np.mean(times["pass_g1"])) / IG_STEPS
    zb_us = float(np.mean(times["pass_mean"]) - np.mean(times[f"pass_g{gdef}"]))
    print(f"per step, one workgroup per graph (pass_g1 / {IG_STEPS}): {step_us:.2f} us")
    print(f"Zb reads (pass_mean - pass_g{gdef}): {zb_us:.2f} us per batch, {100 * zb_us / float(np.mean(times['pass_mean'])):.1f} % of pass_mean")
    n_, o_ = times["api_fused"], times["api_layers"]
    margin = 5 * (max(o_) - min(o_))
    wins = bool(np.mean(o_) - np.mean(n_) > margin)
    print(f"api_fused {np.mean(n_):.1f} us against api_layers {np.mean(o_):.1f} us, 5 x the baseline's spread {margin:.1f} us -> {'fused wins' if wins else 'no win'}")
    print(json.dumps({"bench": "integrated_gradients", "B": B, "steps": IG_STEPS, "reps": args.reps, "runs": args.runs, "rows": rows_j, "fastest_groups": best, "default_groups": attribution.IG_GROUPS_DEFAULT,
                      "step_us": round(step_us, 2), "zb_us": round(zb_us, 2), "fused_wins": wins, "five_spreads_us": round(margin, 2)}))  # fmt: skip


LARGE_B = 8
LARGE_REPS = 10  # calls per timing of --large: the whole run stays well under a minute
LARGE_BARE = 50  # launches of a bare pass per call (a timing window of 10 calls of ~50 us would measure the clock)


def main_large(args):
    """``--large``: input gradients of graphs beyond one workgroup's LDS,
    BASELINE configs[3]-shape synthetic graphs (N 2 700 - 3 300, mean degree
    16.7, 8 - 32 clusters), one batch of ``LARGE_B``.

    * ``api_tiles``      ``input_gradients(model, store, batch, tiles=True)``: one
                         ``dr_ginet_large_input_grad_pass`` (three launches);
    * ``api_layers``     the default call: ``layered.ginet_forward`` with ``x``
                         requiring grad, then ``torch.autograd.grad`` — the only
                         route the parent offers these graphs: the baseline;
    * ``pass_tiles``     the bare ``dr_ginet_large_input_grad_pass``, the handle,
                         the plan and the buffers kept (the two bare passes:
                         ``LARGE_BARE`` launches per call, us per launch);
    * ``pass_large``     the bare ``dr_ginet_large_pass`` with FORWARD | BACKWARD on
                         the same batch and plan: the difference prices the dZ
                         epilogue and the dX kernel."""
    dev = torch.device("cuda:0")
    nb = LARGE_B
    store = GraphStore(pack_graphs(records(make_graphs("atom", nb, 1000))), dev)
    torch.manual_seed(0)
    model = ginet.GINet(30, 1, 3).to(dev).eval()
    idx = np.arange(nb)
    f, xs, out_dim = store.n_feat, store.x_stride, 1

    def api_tiles():
        return attribution.input_gradients(model, store, indices=idx, batch_size=nb, tiles=True)

    def api_layers():
        return attribution.input_gradients(model, store, indices=idx, batch_size=nb)

    a, b = api_tiles(), api_layers()
    assert a.path == "tiles" and b.path == "layers"
    scale = float(b.dx.abs().max())
    assert torch.allclose(a.dx, b.dx, rtol=1e-4, atol=1e-6 * scale) and torch.allclose(a.out, b.out, rtol=1e-4, atol=1e-4), "the two routes agree"

    h = BatchHandle(store, idx.astype(np.int32))
    plan = h.large_plan(out_dim)
    params = [p.detach().contiguous() for p in model.ordered_params()]
    w = ginet.weights_c(params)
    seed = torch.ones(nb, out_dim, device=dev)
    out = torch.empty(nb, out_dim, device=dev)
    slab = torch.empty(nb * ginet.slab_stride(f), device=dev)
    head = torch.zeros(nb * ginet.head_stride(out_dim), device=dev)
    p = make_pass(out_dim, _lib.DR_PASS_FORWARD | _lib.DR_PASS_BACKWARD, dout=seed, out=out, slab=slab, head=head)
    rows = int(a.node_off[-1])
    dx = torch.empty(rows, xs, device=dev)
    dz = torch.empty(rows * (-(-f // 4) * 4), device=dev)
    row_off = torch.from_numpy(a.node_off[:-1].copy()).to(dev)
    ig = _lib.InputGradC()
    ig.dx, ig.row_off, ig.dx_stride = dx.data_ptr(), row_off.data_ptr(), xs
    lib = _lib.load()
    stream = _lib.stream_ptr(dev)

    def pass_tiles():
        _lib.check(lib.dr_ginet_large_input_grad_pass(store.cstruct(), h.descs.data_ptr(), nb, plan.c, w, p, ig, dz.data_ptr(), plan.conv_lds, plan.tail_lds, stream), "dr_ginet_large_input_grad_pass")

    def pass_large():
        _lib.check(lib.dr_ginet_large_pass(store.cstruct(), h.descs.data_ptr(), nb, plan.c, w, p, plan.conv_lds, plan.tail_lds, stream), "dr_ginet_large_pass")

    pass_tiles()
    torch.cuda.synchronize()
    assert torch.equal(dx[:, :f], a.dx), "the bare pass writes the public call's bits"

    n, e, k0 = (v[idx] for v in store._sizes[:3])  # noqa: SLF001
    print(f"B = {nb} atom-level graphs: N {int(n.min())}-{int(n.max())}, E {int(e.min())}-{int(e.max())}, K0 {int(k0.min())}-{int(k0.max())}; tiles of {plan.TILE} rows, {plan.n_tiles} tiles; reps {args.reps} ({args.reps * LARGE_BARE} launches of a bare pass), runs {args.runs}")
    def many(body):
        def run():
            for _ in range(LARGE_BARE):
                body()

        return run

    times = interleaved({"api_tiles": api_tiles, "api_layers": api_layers, "pass_tiles": many(pass_tiles), "pass_large": many(pass_large)}, args.runs, args.reps)
    for name in ("pass_tiles", "pass_large"):
        times[name] = [t / LARGE_BARE for t in times[name]]
    rows_j = []
    print(f"{'variant':>12} {'us/batch':>10} {'spread us':>10}  runs")
    for name, ts in times.items():
        mean, spread = float(np.mean(ts)), float(max(ts) - min(ts))
        rows_j.append({"variant": name, "us": round(mean, 2), "spread_us": round(spread, 2), "runs_us": [round(x, 2) for x in ts]})
        print(f"{name:>12} {mean:10.1f} {spread:10.1f}  {' '.join(f'{x:.1f}' for x in ts)}")
    n_, o_ = times["api_tiles"], times["api_layers"]
    margin = 5 * (max(o_) - min(o_))
    wins = bool(np.mean(o_) - np.mean(n_) > margin)
    print(f"api_tiles {np.mean(n_):.1f} us against api_layers {np.mean(o_):.1f} us, 5 x the baseline's spread {margin:.1f} us -> {'tiles win' if wins else 'no win'}")
    epi = float(np.mean(times["pass_tiles"]) - np.mean(times["pass_large"]))
    print(f"dZ epilogue + dX kernel (pass_tiles - pass_large): {epi:.2f} us per batch")
    print(json.dumps({"bench": "attribution_large", "B": nb, "reps": args.reps, "runs": args.runs, "rows": rows_j, "tiles_win": wins, "five_spreads_us": round(margin, 2), "epilogue_us": round(epi, 2)}))


IG_LARGE_REPS = 3  # calls per timing of --ig --large: the layer route takes about half a second per call
IG_LARGE_BARE = 5  # launches of a bare pass per call


def main_ig_large(args):
    """``--ig --large``: integrated gradients of graphs beyond one workgroup's
    LDS, the ``--large`` batch, 32 Gauss-Legendre nodes, zero baseline.

    * ``pass_gG``        the bare ``dr_ginet_large_integrated_grad_pass`` (all
                         ``2 ceil(32 / G) + 2`` launches) with G groups, G in 1, 2,
                         4, 8, 32, the handle, the plan and the workspaces kept
                         (``IG_LARGE_BARE`` passes per call, us per pass);
    * ``pass_forward``   the bare forward ``dr_ginet_large_pass`` on the same plan
                         (what the public call adds for ``out``);
    * ``api_tiles``      ``integrated_gradients(model, store, batch, tiles=True)``;
    * ``api_layers``     the default call: 32 times ``layered.ginet_forward`` +
                         ``torch.autograd.grad``, the only route the parent offers
                         these graphs: the baseline."""
    dev = torch.device("cuda:0")
    nb = LARGE_B
    store = GraphStore(pack_graphs(records(make_graphs("atom", nb, 1000))), dev)
    torch.manual_seed(0)
    model = ginet.GINet(30, 1, 3).to(dev).eval()
    idx = np.arange(nb)
    f, xs, out_dim = store.n_feat, store.x_stride, 1

    def api_tiles():
        return attribution.integrated_gradients(model, store, indices=idx, batch_size=nb, steps=IG_STEPS, tiles=True)

    def api_layers():
        return attribution.integrated_gradients(model, store, indices=idx, batch_size=nb, steps=IG_STEPS)

    a = api_tiles()
    assert a.path == "tiles"
    if not args.pass_only:  # (a trace holds the tile route's kernels only)
        b = api_layers()
        assert b.path == "layers"
        scale = float(b.attr.abs().max())
        assert torch.allclose(a.attr, b.attr, rtol=1e-4, atol=max(1e-6, 1e-6 * scale)) and torch.allclose(a.out, b.out, rtol=1e-4, atol=1e-4), "the two routes agree"
    print(f"completeness: max |delta| {float(a.delta.abs().max()):.3e} against a mean sum|attr| of {float(a.attr.abs().sum()) / nb:.3e} per graph")

    h = BatchHandle(store, idx.astype(np.int32))
    plan = h.large_plan(out_dim)
    params = [p.detach().contiguous() for p in model.ordered_params()]
    w = ginet.weights_c(params)
    lib = _lib.load()
    stream = _lib.stream_ptr(dev)
    seed = torch.ones(nb, out_dim, device=dev)
    p = make_pass(out_dim, _lib.DR_PASS_FORWARD | _lib.DR_PASS_BACKWARD, dout=seed)
    out = torch.empty(nb, out_dim, device=dev)
    pf = make_pass(out_dim, _lib.DR_PASS_FORWARD, out=out)
    rows = int(a.node_off[-1])
    attr = torch.empty(rows, xs, device=dev)
    off = torch.from_numpy(a.node_off[:-1].copy()).to(dev)
    alpha, weight = torch.from_numpy(a.alpha).to(dev), torch.from_numpy(a.weight).to(dev)
    attr_sum = torch.empty(nb, dtype=torch.float64, device=dev)
    gmax = max(IG_GROUPS)
    slab = torch.empty(gmax * nb * ginet.slab_stride(f), device=dev)
    head = torch.zeros(gmax * nb * ginet.head_stride(out_dim), device=dev)
    outs = torch.empty(gmax * nb * out_dim, device=dev)
    part = torch.empty(gmax, rows, xs, device=dev)
    dz = torch.empty(gmax * rows * (-(-f // 4) * 4), device=dev)
    zg = torch.empty(gmax * rows * xs, device=dev)
    keys = torch.zeros(gmax * nb * plan.k0_max * 32, dtype=torch.int64, device=dev)
    assert plan.c.part_key, "the default plan has keys"

    def bare(groups):
        ig, ws = _lib.IntegratedGradC(), _lib.IgTilesC()
        ig.attr, ig.row_off, ig.dx_stride = attr.data_ptr(), off.data_ptr(), xs
        ig.n_steps, ig.n_groups = IG_STEPS, groups
        ig.alpha, ig.weight = alpha.data_ptr(), weight.data_ptr()
        ig.part, ig.part_off, ig.part_rows = part.data_ptr(), off.data_ptr(), rows
        ig.attr_sum = attr_sum.data_ptr()
        ig.slab, ig.head, ig.out = slab.data_ptr(), head.data_ptr(), outs.data_ptr()
        ws.dz, ws.z, ws.part_key, ws.rows = dz.data_ptr(), zg.data_ptr(), keys.data_ptr(), rows

        def body():
            for _ in range(IG_LARGE_BARE):
                _lib.check(lib.dr_ginet_large_integrated_grad_pass(store.cstruct(), h.descs.data_ptr(), nb, plan.c, w, p, ig, ws, plan.conv_lds, plan.tail_lds, stream), "dr_ginet_large_integrated_grad_pass")

        return body

    def pass_forward():
        for _ in range(IG_LARGE_BARE):
            _lib.check(lib.dr_ginet_large_pass(store.cstruct(), h.descs.data_ptr(), nb, plan.c, w, pf, plan.conv_lds, plan.tail_lds, stream), "dr_ginet_large_pass")

    gdef = min(attribution.IG_TILE_GROUPS_DEFAULT, IG_STEPS)
    bare(gdef)()
    torch.cuda.synchronize()
    assert torch.equal(attr[:, :f], a.attr), "the bare pass writes the public call's bits"

    if args.pass_only:  # for a kernel trace: nothing but bare passes from here on
        body = bare(args.pass_only)
        for _ in range(args.reps):
            body()
        torch.cuda.synchronize()
        print(f"{args.reps * IG_LARGE_BARE} bare passes with {args.pass_only} groups")
        return

    n, e, k0 = (v[idx] for v in store._sizes[:3])  # noqa: SLF001
    print(f"B = {nb} atom-level graphs: N {int(n.min())}-{int(n.max())}, E {int(e.min())}-{int(e.max())}, K0 {int(k0.min())}-{int(k0.max())}; tiles of {plan.TILE} rows, {plan.n_tiles} tiles; S = {IG_STEPS}; reps {args.reps} ({args.reps * IG_LARGE_BARE} bare passes), runs {args.runs}")
    variants = {f"pass_g{g}": bare(g) for g in IG_GROUPS}
    variants["pass_forward"] = pass_forward
    variants["api_tiles"] = api_tiles
    variants["api_layers"] = api_layers
    times = interleaved(variants, args.runs, args.reps)
    for name in times:
        if name.startswith("pass_"):
            times[name] = [t / IG_LARGE_BARE for t in times[name]]
    rows_j = []
    print(f"{'variant':>12} {'us/batch':>12} {'spread us':>10}  runs")
    for name, ts in times.items():
        mean, spread = float(np.mean(ts)), float(max(ts) - min(ts))
        rows_j.append({"variant": name, "us": round(mean, 2), "spread_us": round(spread, 2), "runs_us": [round(x, 2) for x in ts]})
        print(f"{name:>12} {mean:12.1f} {spread:10.1f}  {' '.join(f'{x:.1f}' for x in ts)}")
    best = min(IG_GROUPS, key=lambda g: np.mean(times[f"pass_g{g}"]))
    print(f"fastest groups: {best} (the default is {attribution.IG_TILE_GROUPS_DEFAULT})")
    print(f"per step, one group (pass_g1 / {IG_STEPS}): {float(np.mean(times['pass_g1'])) / IG_STEPS:.2f} us")
    n_, o_ = times["api_tiles"], times["api_layers"]
    margin = 5 * (max(o_) - min(o_))
    wins = bool(np.mean(o_) - np.mean(n_) > margin)
    print(f"api_tiles {np.mean(n_):.1f} us against api_layers {np.mean(o_):.1f} us, 5 x the baseline's spread {margin:.1f} us -> {'tiles win' if wins else 'no win'}")
    print(f"the baseline's spread is {100 * (max(o_) - min(o_)) / np.mean(o_):.1f} % of its mean (wanted: under 10 %)")
    device_us = float(np.mean(times[f"pass_g{gdef}"]) + np.mean(times["pass_forward"]))
    print(f"api_tiles split: device {device_us:.1f} us (pass_g{gdef} + pass_forward), host {float(np.mean(n_)) - device_us:.1f} us (the plan, the workspaces, the launches' enqueue)")
    print(json.dumps({"bench": "integrated_gradients_large", "B": nb, "steps": IG_STEPS, "reps": args.reps, "runs": args.runs, "rows": rows_j, "fastest_groups": best,
                      "default_groups": attribution.IG_TILE_GROUPS_DEFAULT, "tiles_win": wins, "five_spreads_us": round(margin, 2), "device_us": round(device_us, 2)}))  # fmt: skip


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=None, help="calls per timing (default 200: the layer route's timing window is over a second; --large: 10, the layer route is slow on atom-level graphs; --ig --large: 3)")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--ig", action="store_true", help="measure integrated gradients (main_ig) instead of the input gradients")
    ap.add_argument("--large", action="store_true", help="measure the tile route on atom-level graphs (main_large)")
    ap.add_argument("--pass-only", type=int, default=0, metavar="G", help="with --ig --large: after the checks, only --reps x 5 bare passes with G groups (for a kernel trace)")
    args = ap.parse_args()
    args.reps = args.reps or ((IG_LARGE_REPS if args.ig else LARGE_REPS) if args.large else 200)
    if args.ig and args.large:
        main_ig_large(args)
        return
    if args.large:
        main_large(args)
        return
    if args.ig:
        main_ig(args)
        return
    dev = torch.device("cuda:0")
    store = GraphStore(pack_graphs(records(make_graphs("residue", B, 1000))), dev)
    torch.manual_seed(0)
    model = ginet.GINet(30, 1, 3).to(dev).eval()
    idx = np.arange(B)
    f, xs, out_dim = store.n_feat, store.x_stride, 1

    def api_fused():
        return attribution.input_gradients(model, store, indices=idx, batch_size=B, fused=True)

    def api_layers():
        return attribution.input_gradients(model, store, indices=idx, batch_size=B, fused=False)

    a, b = api_fused(), api_layers()
    assert a.path == "fused" and b.path == "layers"
    scale = float(b.dx.abs().max())
    assert torch.allclose(a.dx, b.dx, rtol=1e-4, atol=1e-6 * scale) and torch.allclose(a.out, b.out, rtol=1e-4, atol=1e-4), "the two routes agree"

    # the kept state of the bare launches
    h = BatchHandle(store, idx.astype(np.int32))
    params = [p.detach().contiguous() for p in model.ordered_params()]
    w = ginet.weights_c(params)
    z, zs = store.agg_x(), store.agg_x_stride
    seed = torch.ones(B, out_dim, device=dev)
    out = torch.empty(B, out_dim, device=dev)
    slab = torch.empty(B * ginet.slab_stride(f), device=dev)
    head = torch.zeros(B * ginet.head_stride(out_dim), device=dev)
    p = make_pass(out_dim, _lib.DR_PASS_FORWARD | _lib.DR_PASS_BACKWARD, dout=seed, out=out, slab=slab, head=head)
    dx = torch.empty(int(a.node_off[-1]), xs, device=dev)
    row_off = torch.from_numpy(a.node_off[:-1].copy()).to(dev)
    ig = _lib.InputGradC()
    ig.dx, ig.row_off, ig.dx_stride = dx.data_ptr(), row_off.data_ptr(), xs
    lib = _lib.load()
    alias = int(store.packed.transpose_aliased)
    lds_ig = int(lib.dr_ginet_input_grad_lds_bytes(*h.max_sizes[:2], f, *h.max_sizes[2:], alias, out_dim, zs))
    lds_z = z_lds_for(h, out_dim)
    stream = _lib.stream_ptr(dev)

    def launch_ig():
        _lib.check(lib.dr_ginet_input_grad_pass(store.cstruct(), h.descs.data_ptr(), B, w, p, ig, z.data_ptr(), zs, lds_ig, stream), "dr_ginet_input_grad_pass")

    def launch_pass_z():
        _lib.check(lib.dr_ginet_graph_pass_z(store.cstruct(), h.descs.data_ptr(), B, w, p, lds_z, z.data_ptr(), zs, stream), "dr_ginet_graph_pass_z")

    t = copy.copy(layered.batch_tensors(h))
    t.x = t.x.detach().clone().requires_grad_(True)

    def layers_steady():
        o = layered.ginet_forward(model, t, training=False)
        return torch.autograd.grad((o * seed).sum(), t.x)

    launch_ig()
    torch.cuda.synchronize()
    assert torch.equal(dx[:, :f], a.dx), "the bare launch writes the public call's bits"

    times = interleaved({"api_fused": api_fused, "api_layers": api_layers, "launch_ig": launch_ig, "launch_pass_z": launch_pass_z, "layers_steady": layers_steady}, args.runs, args.reps)
    rows = []
    print(f"{'variant':>14} {'us/batch':>10} {'spread us':>10}  runs")
    for name, ts in times.items():
        mean, spread = float(np.mean(ts)), float(max(ts) - min(ts))
        rows.append({"variant": name, "us": round(mean, 2), "spread_us": round(spread, 2), "runs_us": [round(x, 2) for x in ts]})
        print(f"{name:>14} {mean:10.1f} {spread:10.1f}  {' '.join(f'{x:.1f}' for x in ts)}")
    verdicts = []
    for new, old in (("api_fused", "api_layers"), ("launch_ig", "layers_steady")):
        n_, o_ = times[new], times[old]
        margin = 5 * (max(o_) - min(o_))
        wins = bool(np.mean(o_) - np.mean(n_) > margin)
        verdicts.append({"fused": new, "baseline": old, "fused_us": round(float(np.mean(n_)), 2), "baseline_us": round(float(np.mean(o_)), 2), "five_spreads_us": round(margin, 2), "fused_wins": wins})
        print(f"{new} {np.mean(n_):.1f} us against {old} {np.mean(o_):.1f} us, 5 x the baseline's spread {margin:.1f} us -> {'fused wins' if wins else 'no win'}")
    epi = float(np.mean(times["launch_ig"]) - np.mean(times["launch_pass_z"]))
    print(f"epilogue (launch_ig - launch_pass_z): {epi:.2f} us per batch")
    print(json.dumps({"bench": "attribution", "B": B, "reps": args.reps, "runs": args.runs, "rows": rows, "verdicts": verdicts, "epilogue_us": round(epi, 2)}))


if __name__ == "__main__":
    main()
