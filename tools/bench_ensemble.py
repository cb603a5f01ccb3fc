"""Measurement: K GINet members stepped by one pair of launches
(``FusedEnsembleStep``) against the same K members stepped one after another
(``FusedTrainStep``, what training K models costs without it).

configs[1]-shape synthetic graphs, B = 64 per member, K in {1, 2, 4, 8}, the
members on the same batch (a true ensemble) and on distinct batches (folds).
Every variant is captured into a HIP graph holding ``--steps`` steps and timed
over ``--reps`` replays between two device events:

* ``ensemble``     one captured ensemble step (2 launches for K members);
* ``sequential``   K captured single-model steps back to back in one graph
                   (2 K launches; the strongest form of the baseline);
* ``k_graphs``     K single-model graphs replayed one after another (the same
                   launches plus a graph launch per member).

The variants are interleaved in one process and each runs ``--runs`` times; the
table gives the mean us per ensemble step (all K members advance one step), the
same per member-step, and the spread (max - min) over the runs.
"""

from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "deeprank-gnn-2_amd")]

from bench import make_graphs, records  # noqa: E402
from deeprank2_amd.engine import FusedTrainStep  # noqa: E402
from deeprank2_amd.ensemble import FusedEnsembleStep  # noqa: E402
from deeprank2_amd.fused import BatchHandle  # noqa: E402
from deeprank2_amd.neuralnets.gnn.ginet import GINet  # noqa: E402
from deeprank2_amd.store import GraphStore, pack_graphs  # noqa: E402

B = 64


def replay_us(graphs, steps, reps):
    """us per step of ``reps`` rounds over ``graphs`` (each holding ``steps`` steps), device events."""
    for g in graphs:
        g.replay()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        for g in graphs:
            g.replay()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / (reps * steps)


def capture(body, steps):
    body()  # warm-up: Z, argument buffers, LDS attributes
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(steps):
            body()
    torch.cuda.synchronize()
    return g


def models(k, dev):
    out = []
    for i in range(k):
        torch.manual_seed(i)
        out.append(GINet(30, 1, 3).to(dev).train())
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--members", type=int, nargs="+", default=[1, 2, 4, 8])
    ap.add_argument("--steps", type=int, default=10, help="steps held by each captured graph")
    ap.add_argument("--reps", type=int, default=100, help="replays per timing")
    ap.add_argument("--runs", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    kmax = max(args.members)
    store = GraphStore(pack_graphs(records(make_graphs("residue", kmax * B, 1000))), dev)
    rows = []
    print(f"{'K':>2} {'batches':>8} {'variant':>10} {'us/ens-step':>12} {'us/member-step':>15} {'spread us':>10}  runs")
    for k in args.members:
        for mode in ("same", "distinct"):
            if k == 1 and mode == "distinct":
                continue
            hs = [BatchHandle(store, np.arange(B, dtype=np.int32) + (i * B if mode == "distinct" else 0)) for i in range(k)]
            ens = FusedEnsembleStep(models(k, dev))
            singles = [FusedTrainStep(m) for m in models(k, dev)]
            g_ens = capture(lambda: ens.step(hs), args.steps)  # noqa: B023
            assert ens.last_path == "fused"

            def seq():
                for st, h in zip(singles, hs):  # noqa: B023
                    st.step(h)

            g_seq = capture(seq, args.steps)
            g_each = [capture(lambda st=st, h=h: st.step(h), args.steps) for st, h in zip(singles, hs)]
            variants = {"ensemble": [g_ens], "sequential": [g_seq], "k_graphs": g_each}
            times = {name: [] for name in variants}
            for _ in range(args.runs):
                for name, graphs in variants.items():
                    times[name].append(replay_us(graphs, args.steps, args.reps))
            for name, t in times.items():
                mean, spread = float(np.mean(t)), float(max(t) - min(t))
                rows.append({"K": k, "batches": mode, "variant": name, "us_per_ensemble_step": round(mean, 3), "us_per_member_step": round(mean / k, 3), "spread_us": round(spread, 3), "runs_us": [round(x, 3) for x in t]})
                print(f"{k:>2} {mode:>8} {name:>10} {mean:12.2f} {mean / k:15.2f} {spread:10.2f}  {' '.join(f'{x:.2f}' for x in t)}")
            finite = all(bool(torch.isfinite(p).all()) for st in [*ens.steps, *singles] for p in st.params)
            assert finite, "a member's parameters left the finite range during the timed steps"
    print(json.dumps({"bench": "ensemble", "B": B, "steps_per_graph": args.steps, "reps": args.reps, "rows": rows}))


if __name__ == "__main__":
    main()
