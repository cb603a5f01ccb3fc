"""Measurement: the forward side of an ensemble (``FusedEnsembleForward``)
against what it replaces.

configs[1]-shape synthetic graphs, B = 64.

(a) One validation phase of K = 2, 4, 8 folds with 256 held-out graphs per
    member (4 batches each), as ``train_ensemble`` runs it after every epoch,
    from the first launch to the K losses on the host:

    * ``parent``    the per-member loop ``_held_out_loss``: K x 4 eager
                    ``model(batch)`` calls, one 64-workgroup launch each;
    * ``eager``     the fused runner issuing its 4 launches (grids (64, K));
    * ``captured``  the same launches replayed as one HIP graph (the default);
    * ``device_loss``  captured, with ``val_loss="device"``: the graph ends with
                    one ``dr_ensemble_score`` launch and the phase with one
                    copy of K rows of doubles (no torch loss call).

(b) ``predict_ensemble`` over 1 024 graphs for K = 1, 4, 8 (16 multi-member
    launches in one graph, the statistics launch, a copy of the predictions)
    against K ``EvalRunner``s replayed one after another (K graphs of 16
    launches; no statistics).

Wall-clock us per phase / per call, each ending with the device idle (``--reps``
calls per timing).  The variants are interleaved in one process and each runs
``--runs`` times; the table gives the mean and the spread (max - min) over the
runs.  The last lines state, per K, whether the captured runner beats the
parent's path by more than five times that path's own spread, and whether the
device loss beats the captured runner's host loss by five times that one's.
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "deeprank-gnn-2_amd")]

from bench import make_graphs, records  # noqa: E402
from deeprank2_amd import ensemble  # noqa: E402
from deeprank2_amd.ensemble import FusedEnsembleStep, epoch_batches, predict_ensemble  # noqa: E402
from deeprank2_amd.epoch import EvalRunner  # noqa: E402
from deeprank2_amd.neuralnets.gnn.ginet import GINet  # noqa: E402
from deeprank2_amd.store import GraphStore, pack_graphs  # noqa: E402

B = 64
HELD_OUT = 256
PREDICT = 1024


def wall_us(body, reps):
    """us per call of ``reps`` calls of ``body``, the device idle before and after."""
    body()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        body()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / reps


def models(k, dev, train):
    out = []
    for i in range(k):
        torch.manual_seed(i)
        out.append(GINet(30, 1, 3).to(dev).train(train))
    return out


def interleaved(variants, runs, reps):
    times = {name: [] for name in variants}
    for _ in range(runs):
        for name, body in variants.items():
            times[name].append(wall_us(body, reps))
    return times


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--folds", type=int, nargs="+", default=[2, 4, 8])
    ap.add_argument("--members", type=int, nargs="+", default=[1, 4, 8])
    ap.add_argument("--reps", type=int, default=20, help="calls per timing")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--what", choices=["both", "validate", "predict"], default="both", help="table (a), table (b), or both")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    n_graphs = max(max(args.folds) * HELD_OUT, PREDICT)
    store = GraphStore(pack_graphs(records(make_graphs("residue", n_graphs, 1000))), dev)
    rows, verdicts = [], []
    print(f"{'what':>8} {'K':>2} {'variant':>12} {'us':>10} {'spread us':>10}  runs")

    def report(what, k, times):
        for name, t in times.items():
            mean, spread = float(np.mean(t)), float(max(t) - min(t))
            rows.append({"what": what, "K": k, "variant": name, "us": round(mean, 2), "spread_us": round(spread, 2), "runs_us": [round(x, 2) for x in t]})
            print(f"{what:>8} {k:>2} {name:>12} {mean:10.1f} {spread:10.1f}  {' '.join(f'{x:.1f}' for x in t)}")

    # (a) the validation phase of K folds
    for k in args.folds if args.what != "predict" else []:
        ens = FusedEnsembleStep(models(k, dev, True), max_batch=B)
        val_idx = [np.arange(m * HELD_OUT, (m + 1) * HELD_OUT) for m in range(k)]
        captured = ensemble._HeldOut(ens, store, val_idx, B, fused=True)  # noqa: SLF001
        eager = ensemble._HeldOut(ens, store, val_idx, B, fused=True)  # noqa: SLF001
        eager.runner.captured = False
        device = ensemble._HeldOut(ens, store, val_idx, B, fused=True, device_loss=True)  # noqa: SLF001

        def device_loss():
            return device.scores().loss  # noqa: B023

        def parent():
            return [ensemble._held_out_loss(st, store, v, B) for st, v in zip(ens.steps, val_idx)]  # noqa: SLF001, B023

        ref = parent()
        for held in (captured, eager):
            assert held.losses().tolist() == ref and held.runner.last_path == "fused", "the runner's losses are the parent loop's"
        assert captured.runner.graph is not None and eager.runner.graph is None
        np.testing.assert_allclose(device_loss(), ref, rtol=1e-5, err_msg="the device loss is the host's up to rounding")
        assert device.runner.last_path == "fused" and device.runner.graph is not None
        times = interleaved({"parent": parent, "eager": eager.losses, "captured": captured.losses, "device_loss": device_loss}, args.runs, args.reps)
        report("validate", k, times)
        p, c = times["parent"], times["captured"]
        margin = 5 * (max(p) - min(p))
        verdicts.append({"what": "validate", "K": k, "parent_us": round(float(np.mean(p)), 2), "captured_us": round(float(np.mean(c)), 2), "five_spreads_us": round(margin, 2), "captured_wins": bool(np.mean(p) - np.mean(c) > margin)})
        d, margin = times["device_loss"], 5 * (max(c) - min(c))  # the yardstick: the captured runner with the host loss
        verdicts.append({"what": "val_loss", "K": k, "parent_us": round(float(np.mean(c)), 2), "captured_us": round(float(np.mean(d)), 2), "five_spreads_us": round(margin, 2), "captured_wins": bool(np.mean(c) - np.mean(d) > margin)})

    # (b) predict_ensemble against K EvalRunners in turn
    idx = np.arange(PREDICT)
    batches = epoch_batches(idx, B, False, 0, 0, 0)
    for k in args.members if args.what != "validate" else []:
        ms = models(k, dev, False)
        runners = [EvalRunner(m, store, [len(b) for b in batches]) for m in ms]

        def each():
            return [r.run(batches) for r in runners]  # noqa: B023

        def predict():
            return predict_ensemble(ms, store, indices=idx, batch_size=B)  # noqa: B023

        pred = predict()
        assert all(torch.equal(pred.members[m], o) for m, o in enumerate(each())), "the ensemble's rows are the EvalRunners'"
        times = interleaved({"eval_runners": each, "predict": predict}, args.runs, args.reps)
        report("predict", k, times)
        p, c = times["eval_runners"], times["predict"]
        margin = 5 * (max(p) - min(p))
        verdicts.append({"what": "predict", "K": k, "parent_us": round(float(np.mean(p)), 2), "captured_us": round(float(np.mean(c)), 2), "five_spreads_us": round(margin, 2), "captured_wins": bool(np.mean(p) - np.mean(c) > margin)})

    for v in verdicts:
        if v["what"] == "val_loss":
            print(f"{v['what']:>8} K={v['K']}: captured, host loss {v['parent_us']:.1f} us, captured, device loss {v['captured_us']:.1f} us, 5 x the host loss's spread {v['five_spreads_us']:.1f} us -> {'device loss wins' if v['captured_wins'] else 'no win'}")
            continue
        print(f"{v['what']:>8} K={v['K']}: parent {v['parent_us']:.1f} us, fused+captured {v['captured_us']:.1f} us, 5 x parent's spread {v['five_spreads_us']:.1f} us -> {'fused wins' if v['captured_wins'] else 'no win'}")
    print(json.dumps({"bench": "ensemble_forward", "B": B, "held_out_per_member": HELD_OUT, "predict_graphs": PREDICT, "reps": args.reps, "runs": args.runs, "rows": rows, "verdicts": verdicts}))


if __name__ == "__main__":
    main()
