"""GPU parity of the fused training step under AdamW / Adamax
(``dr_reduce_update_opt``) and the L1 / SmoothL1 / Huber losses (DR_LOSS_L1 /
DR_LOSS_SMOOTH_L1 / DR_LOSS_HUBER in every graph pass): the update rules
against torch's optimizers, the losses against the CPU oracle
(oracle/gnn_ref.py) plus torch's loss functions, and the Trainer end to end
on the reference's documented ``configure_optimizers(torch.optim.Adamax, ...)``;
last, the reduce launch alone on a synthetic table (section 7).
Tolerances: 1e-4 on outputs / losses / gradients (north_star, fp32), rtol
1e-5 + atol 1e-7 on the update (test_gpu_ginet.py's figure)."""

from __future__ import annotations

import ctypes
import functools

import numpy as np
import pytest
import torch
from _util import assert_grad_close
from torch import nn

from deeprank2_amd import _lib
from deeprank2_amd.dataset import GraphDataset
from deeprank2_amd.engine import FusedTrainStep
from deeprank2_amd.exporters import MemoryOutputExporter
from deeprank2_amd.fused import BatchHandle
from deeprank2_amd.neuralnets.gnn import foutnet as fout_amd
from deeprank2_amd.neuralnets.gnn import ginet as ginet_amd
from deeprank2_amd.neuralnets.gnn import ginet_nocluster as nc_amd
from deeprank2_amd.neuralnets.gnn import sgat as sgat_amd
from deeprank2_amd.neuralnets.gnn import vanilla_gnn as van_amd
from deeprank2_amd.store import GraphStore, pack_graphs, records_from_batch
from deeprank2_amd.trainer import Trainer
from deeprank2_amd.utils import synthetic as S
from oracle import data_ref, gnn_ref
from oracle import pyg_ops as P

pytestmark = pytest.mark.gpu
TOL = dict(rtol=1e-4, atol=1e-4)
UPD = dict(rtol=1e-5, atol=1e-7)
DEV = "cuda:0"

# name -> (oracle class, MI355X class, parameter names, constructor arguments)
MODELS = {
    "ginet": (gnn_ref.GINet, ginet_amd.GINet, ginet_amd.PARAM_NAMES, (30, 1, 3)),
    "foutnet": (gnn_ref.FoutNet, fout_amd.FoutNet, fout_amd.PARAM_NAMES, (30, 1)),
    "sgat": (gnn_ref.SGAT, sgat_amd.SGAT, sgat_amd.PARAM_NAMES, (30, 1)),
    "nocluster": (gnn_ref.GINetNoCluster, nc_amd.GINet, nc_amd.PARAM_NAMES, (30, 1, 3)),
    "vanilla": (gnn_ref.VanillaNetwork, van_amd.VanillaNetwork, van_amd.PARAM_NAMES, (30, 1, 3)),
}
# (data seed, model seed) per model, chosen on the CPU so that the oracle's
# residuals satisfy _check_residuals for every new loss
SEEDS = {"ginet": (1, 1), "foutnet": (1, 1), "sgat": (1, 2), "nocluster": (1, 1), "vanilla": (1, 1)}


def _connected(graphs):
    """The graphs whose every depth-0 cluster has a pooled edge (FoutNet's conv2
    makes an isolated pooled node NaN, foutnet.py:58)."""
    out = []
    for g in graphs:
        c = g["cluster0"][g["index"]]
        cross = c[:, 0] != c[:, 1]
        if np.unique(c[cross]).size == int(g["cluster0"].max()) + 1:
            out.append(g)
    return out


def _datas(name, n, seed):
    """n synthetic graphs of 25-60 nodes (F=30, Fe=3) as the oracle's Data, shaped for model `name`."""
    graphs = _connected(S.make_dataset(6 * n, seed=seed, n_lo=25, n_hi=60))[:n]
    assert len(graphs) == n
    datas = [data_ref.synthetic_to_data(g, f"{name}{i}") for i, g in enumerate(graphs)]
    for d in datas:
        if name == "sgat":  # SGAT multiplies its one edge feature into every channel (sgat.py:71)
            d.edge_attr = d.edge_attr[:, :1].contiguous()
        if name == "vanilla":
            d.cluster0 = d.cluster1 = None
    return datas


def _store(name, datas):
    return GraphStore(pack_graphs(records_from_batch(P.Batch.from_data_list(datas)), require_clusters=name != "vanilla"), DEV)


def _oracle_model(name, seed):
    torch.manual_seed(seed)
    return MODELS[name][0](*MODELS[name][3]).eval()  # eval: dropout off (GINet's p = 0.4)


def _gpu_model(name, model_o):
    m = MODELS[name][1](*MODELS[name][3])
    m.load_state_dict(model_o.state_dict())
    return m.to(DEV).train()


def _torch_loss(loss, param):
    if loss == "l1":
        return nn.L1Loss()
    return nn.SmoothL1Loss(beta=param) if loss == "smooth_l1" else nn.HuberLoss(delta=param)


@functools.lru_cache(maxsize=None)
def _oracle_case(name, n=6):
    """The oracle's forward on the model's seeded batch, computed once: (datas,
    model, out [n], |out - y| [n])."""
    dseed, mseed = SEEDS[name]
    datas = _datas(name, n, dseed)
    model_o = _oracle_model(name, mseed)
    bat = P.Batch.from_data_list([d.clone() for d in datas])
    with torch.no_grad():
        out = model_o(bat).reshape(-1)
    return datas, model_o, out, (out - bat.y).abs().numpy()


def _check_residuals(ad, loss, thr):
    """The batch exercises both branches of the loss, away from the points
    where fp32 differences between the kernel and the oracle could flip one."""
    assert np.isfinite(ad).all()
    if loss == "l1":
        assert (ad >= 1e-3).all(), ad
        return
    assert (ad < thr).sum() >= 2 and (ad > thr).sum() >= 2, (ad, thr)
    assert (np.abs(ad - thr) > 0.01 * thr).all(), (ad, thr)


def _oracle_grads(name, loss, param):
    datas, model_o, _, _ = _oracle_case(name)
    model_o.zero_grad()
    bat = P.Batch.from_data_list([d.clone() for d in datas])
    out = model_o(bat)
    lo = _torch_loss(loss, param)(out.reshape(-1), bat.y)
    lo.backward()
    return out.detach(), float(lo.detach()), {n: p.grad.clone() for n, p in model_o.named_parameters()}


def _check_step_vs_oracle(name, loss, param, step, h, ntol=1e-6):
    out_o, loss_o, grads_o = _oracle_grads(name, loss, param)
    lo, out = step.step(h, dropout=False)
    torch.cuda.synchronize()
    np.testing.assert_allclose(out.cpu().numpy(), out_o.numpy(), **TOL)
    assert float(lo) == pytest.approx(loss_o, rel=1e-4)
    grads = dict(zip(MODELS[name][2], step.grads))
    for n, g in grads_o.items():
        assert_grad_close(grads[n].cpu().numpy(), g.numpy(), ntol=ntol, err_msg=f"{name} {loss} {n}")


# ---------------------------------------------------------------- 1. update rule
def _update_case(name, b, kind):
    """Three consecutive steps of `kind` on b graphs of model `name`, each
    compared with the torch optimizer fed the kernel's own gradients."""
    lr, wd = 1e-3, 1e-2
    dseed, mseed = SEEDS[name]
    datas = _datas(name, b, dseed)
    model_o = _oracle_model(name, mseed)
    model = _gpu_model(name, model_o)
    h = BatchHandle(_store(name, datas), np.arange(b))
    step = FusedTrainStep(model, lr=lr, weight_decay=wd, optimizer=kind)
    names = MODELS[name][2]
    ref = [nn.Parameter(p.detach().cpu().clone()) for p in step.params]
    cls, second = {"adamw": (torch.optim.AdamW, "exp_avg_sq"), "adamax": (torch.optim.Adamax, "exp_inf")}[kind]
    opt = cls(ref, lr=lr, weight_decay=wd, foreach=False)
    l2 = [nn.Parameter(r.detach().clone()) for r in ref]  # the same inputs under Adam with L2 decay
    opt_l2 = torch.optim.Adam(l2, lr=lr, weight_decay=wd, foreach=False)
    shrunk = 0
    for it in range(3):
        before = [p.detach().cpu().clone() for p in step.params]
        if name == "vanilla" and it == 1:
            # the packed weight copy the pass reads was rewritten by step 1's
            # update: step 2's outputs are the oracle's on torch's parameters
            with torch.no_grad():
                for n, po in model_o.named_parameters():
                    po.copy_(ref[names.index(n)])
                out_o = model_o(P.Batch.from_data_list([d.clone() for d in datas]))
        _, out = step.step(h, dropout=False)
        torch.cuda.synchronize()
        if name == "vanilla" and it == 1:
            np.testing.assert_allclose(out.cpu().numpy(), out_o.numpy(), **TOL)
        for r, q, g in zip(ref, l2, step.grads):
            r.grad = g.detach().cpu().clone()
            q.grad = g.detach().cpu().clone()
        opt.step()
        opt_l2.step()
        for n, r, p, (m, v), g, p0 in zip(names, ref, step.params, step.states, step.grads, before):
            what = f"{name} {kind} {n} step {it}"
            np.testing.assert_allclose(p.detach().cpu().numpy(), r.detach().numpy(), err_msg=what, **UPD)
            np.testing.assert_allclose(m.cpu().numpy(), opt.state[r]["exp_avg"].numpy(), err_msg=what, **UPD)
            np.testing.assert_allclose(v.cpu().numpy(), opt.state[r][second].numpy(), err_msg=what, **UPD)
            if kind == "adamw" and not bool(g.any()):  # GINet's attention weights: decay alone
                np.testing.assert_allclose(p.detach().cpu().numpy(), (p0 * (1.0 - lr * wd)).numpy(), err_msg=what, **UPD)
                shrunk += 1
        assert int(step.counter[0].item()) == it + 1
    if kind == "adamw":
        if name in ("ginet", "nocluster"):
            assert shrunk >= 3
        # a decay rule mistaken for Adam's L2 term would not pass the comparison above
        mine = np.concatenate([p.detach().cpu().numpy().ravel() for p in step.params])
        other = np.concatenate([q.detach().numpy().ravel() for q in l2])
        assert not np.allclose(mine, other, **UPD)
        assert float(np.max(np.abs(mine - other) - (UPD["atol"] + UPD["rtol"] * np.abs(other)))) > 1e-5
    return {p.numel() for p in step.params}


@pytest.mark.parametrize("kind", ["adamw", "adamax"])
@pytest.mark.parametrize(("name", "b"), [("foutnet", 6), ("ginet", 6), ("vanilla", 4), ("foutnet", 1)])
def test_update_rule_matches_torch_for_three_steps(name, b, kind):
    sizes = _update_case(name, b, kind)
    assert 1 in sizes  # fc2.bias: one live lane in its block
    if name == "ginet":
        assert 9 in sizes  # conv*.fc_edge_attr.weight


# ------------------------------------------------------------ 2. loss vs oracle
LOSSES = ["l1", "smooth_l1", "huber"]


def _param_for(name, loss):
    _, _, _, ad = _oracle_case(name)
    thr = None if loss == "l1" else float(np.median(ad))
    _check_residuals(ad, loss, thr)
    return thr


@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("name", list(MODELS))
def test_loss_step_matches_oracle(name, loss):
    param = _param_for(name, loss)
    datas, model_o, _, _ = _oracle_case(name)
    h = BatchHandle(_store(name, datas), np.arange(len(datas)))
    if name == "vanilla":
        assert van_amd.fused_fits(h, 30, 3)  # the per-graph kernel (vanilla_graph.hip)
    step = FusedTrainStep(_gpu_model(name, model_o), loss=loss, loss_param=param)
    _check_step_vs_oracle(name, loss, param, step, h)


@pytest.mark.parametrize("path", ["large", "acc", "layers"])
def test_huber_on_every_ginet_path(path):
    param = _param_for("ginet", "huber")
    datas, model_o, _, _ = _oracle_case("ginet")
    h = BatchHandle(_store("ginet", datas), np.arange(len(datas)))
    step = FusedTrainStep(_gpu_model("ginet", model_o), loss="huber", loss_param=param)
    if path == "large":
        h.force_large = True  # tile + tail launches
    elif path == "layers":
        h.force_layers = True  # layer-level forward, torch.nn.functional loss
    else:
        step.acc, step.acc_groups = True, 2  # the accumulating pass: loss summed on chip
    _check_step_vs_oracle("ginet", "huber", param, step, h)
    assert (step._acc_slab is not None) == (path == "acc")  # noqa: SLF001


@pytest.mark.parametrize("loss", LOSSES)
def test_loss_on_the_vanilla_chunk_pipeline(loss):
    param = _param_for("vanilla", loss)
    datas, model_o, _, _ = _oracle_case("vanilla")
    h = BatchHandle(_store("vanilla", datas), np.arange(len(datas)))
    h.vanilla_pipeline = True  # dr_vanilla_graph_pass (vanilla_fused.hip)
    step = FusedTrainStep(_gpu_model("vanilla", model_o), loss=loss, loss_param=param)
    _check_step_vs_oracle("vanilla", loss, param, step, h)


@pytest.mark.parametrize("name", ["foutnet", "sgat", "nocluster"])
def test_huber_on_the_large_graph_passes(name):
    param = _param_for(name, "huber")
    datas, model_o, _, _ = _oracle_case(name)
    h = BatchHandle(_store(name, datas), np.arange(len(datas)))
    h.force_large = True
    step = FusedTrainStep(_gpu_model(name, model_o), loss="huber", loss_param=param)
    _check_step_vs_oracle(name, "huber", param, step, h)


def test_smooth_l1_beta_zero_is_l1():
    _param_for("foutnet", "l1")
    datas, model_o, _, _ = _oracle_case("foutnet")
    h = BatchHandle(_store("foutnet", datas), np.arange(len(datas)))
    step = FusedTrainStep(_gpu_model("foutnet", model_o), loss="smooth_l1", loss_param=0.0)
    _check_step_vs_oracle("foutnet", "smooth_l1", 0.0, step, h)


# ---------------------------------------------------------------- 3. non-finite
@pytest.mark.parametrize("loss", LOSSES)
def test_nan_output_gives_nan_loss_and_torchs_gradient(loss):
    """Graph 0 pooled into ONE depth-0 cluster: the pooled node has no
    out-edge, FoutLayer's mean over nothing is NaN (foutnet.py:58) and so is
    the graph's output.  The loss is NaN; the gradient is torch's (sign(NaN) =
    0 for L1 -- the other graphs' finite gradients remain --, NaN otherwise)."""
    datas = _datas("foutnet", 6, 11)
    datas[0].cluster0 = torch.zeros_like(datas[0].cluster0)
    datas[0].cluster1 = torch.zeros(1, dtype=torch.long)
    model_o = _oracle_model("foutnet", 9)
    bat = P.Batch.from_data_list([d.clone() for d in datas])
    out_o = model_o(bat)
    assert torch.isnan(out_o[0]).all() and torch.isfinite(out_o[1:]).all()
    lo = _torch_loss(loss, 0.5)(out_o.reshape(-1), bat.y)
    lo.backward()
    assert torch.isnan(lo)
    step = FusedTrainStep(_gpu_model("foutnet", model_o), loss=loss, loss_param=0.5)
    h = BatchHandle(_store("foutnet", datas), np.arange(6))
    loss_k, out = step.step(h)
    torch.cuda.synchronize()
    assert torch.isnan(loss_k).all()
    np.testing.assert_allclose(out.cpu().numpy(), out_o.detach().numpy(), equal_nan=True, **TOL)
    grads = dict(zip(fout_amd.PARAM_NAMES, step.grads))
    for n, p in model_o.named_parameters():
        g, r = grads[n].cpu().numpy(), p.grad.numpy()
        np.testing.assert_array_equal(np.isnan(g), np.isnan(r), err_msg=n)
        assert_grad_close(g, r, err_msg=n)
    fc2b = grads["fc2.bias"].cpu().numpy()
    assert np.isfinite(fc2b).all() if loss == "l1" else np.isnan(fc2b).all()


# ------------------------------------------------------------- 4. Trainer e2e
def _connected_clusters(n, seed):
    out, s = [], seed
    while len(out) < n:
        out += _connected(S.make_dataset(4 * n, seed=s, n_lo=25, n_hi=60, mean_degree=8.0))
        s += 1000
    return out[:n]


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("optl")
    tr, va = str(d / "train.hdf5"), str(d / "valid.hdf5")
    S.write_hdf5(tr, _connected_clusters(24, 11), prefix="tr")
    S.write_hdf5(va, _connected_clusters(8, 12), prefix="va")
    return tr, va


def _sets(tr_path, va_path):
    tr = GraphDataset(tr_path, node_features=S.SYNTH_NODE_FEATURES, edge_features=S.SYNTH_EDGE_FEATURES, target="irmsd", clustering_method="mcl")
    return tr, GraphDataset(va_path, train_source=tr, clustering_method="mcl")


def _oracle_batch(ds, idx):
    datas = []
    for i in idx:
        d = ds.get(i)
        o = P.Data(x=d.x, edge_index=d.edge_index, edge_attr=d.edge_attr, y=d.y, pos=d.pos)
        o.cluster0, o.cluster1 = d.cluster0, d.cluster1
        datas.append(o)
    return P.Batch.from_data_list(datas)


def _losses(mem, phase):
    return [r["loss"] for r in mem.records if r["phase"] == phase]


def _replay(model_o, opt, lossfn, tr, va, nepoch, bs):
    """The reference loop (trainer.py:503-724) on the oracle: epoch-0
    evaluations, then one training and one validation pass per epoch."""
    losses = {"training": [], "validation": []}

    def ev(ds):
        model_o.eval()
        tot, n = 0.0, 0
        with torch.no_grad():
            for s in range(0, len(ds), bs):
                b = _oracle_batch(ds, range(s, min(s + bs, len(ds))))
                out = model_o(b).reshape(-1)
                tot += float(lossfn(out, b.y)) * out.shape[0]
                n += out.shape[0]
        return tot / n

    losses["training"].append(ev(tr))
    losses["validation"].append(ev(va))
    for _ in range(nepoch):
        model_o.train()
        tot, n = 0.0, 0
        for s in range(0, len(tr), bs):
            b = _oracle_batch(tr, range(s, min(s + bs, len(tr))))
            opt.zero_grad()
            out = model_o(b).reshape(-1)
            loss = lossfn(out, b.y)
            loss.backward()
            opt.step()
            tot += float(loss.detach()) * out.shape[0]
            n += out.shape[0]
        losses["training"].append(tot / n)
        losses["validation"].append(ev(va))
    return losses


def test_trainer_adamax_huber_fused_matches_oracle_replay(files, tmp_path):
    """The reference's documented optimizer line (README: Adamax, lr=0.001,
    weight_decay=1e-4) with HuberLoss on FoutNet: the fused path runs, the
    epoch losses and final parameters follow an oracle replay, the checkpoint
    is torch.optim.Adamax's and a Trainer restarted from it continues fused
    exactly where the first one would."""
    tr, va = _sets(*files)
    mem = MemoryOutputExporter()
    torch.manual_seed(4)
    t = Trainer(FoutNet := fout_amd.FoutNet, tr, va, cuda=True, output_exporters=[mem], precluster=False)
    t.configure_optimizers(torch.optim.Adamax, lr=0.001, weight_decay=1e-04)
    t.set_lossfunction(nn.HuberLoss)
    model_o = gnn_ref.FoutNet(30, 1)
    model_o.load_state_dict({k: v.cpu() for k, v in t.model.state_dict().items()})
    path = str(tmp_path / "adamax.pth.tar")
    t.train(nepoch=3, batch_size=8, shuffle=False, validate=True, best_model=False, filename=path)
    assert t._fused and t._fused.optimizer == "adamax" and t._fused.loss == "huber"  # noqa: SLF001
    assert np.isfinite(_losses(mem, "training")).all()
    ref = _replay(model_o, torch.optim.Adamax(model_o.parameters(), lr=0.001, weight_decay=1e-04), nn.HuberLoss(), tr, va, 3, 8)
    np.testing.assert_allclose(_losses(mem, "training"), ref["training"], rtol=2e-4)
    np.testing.assert_allclose(_losses(mem, "validation"), ref["validation"], rtol=2e-4)
    for n, p in model_o.named_parameters():
        mine = t.model.state_dict()[n].cpu().numpy()
        assert np.mean(np.abs(mine - p.detach().numpy()) < 1e-5) > 0.97, n
    # the checkpoint names Adamax and holds its state after 3 epochs x 3 batches
    state = torch.load(path, weights_only=True)
    assert state["optimizer"] == "Adamax" and state["lossfunction"] == "HuberLoss"
    probe = torch.optim.Adamax([nn.Parameter(v.clone()) for v in state["model_state"].values()])
    probe.load_state_dict(state["optimizer_state"])
    st0 = probe.state[probe.param_groups[0]["params"][0]]
    assert int(float(st0["step"])) == 9 and set(st0) == {"step", "exp_avg", "exp_inf"}
    assert probe.param_groups[0]["weight_decay"] == 1e-04
    # restart from the file: fused again, and one more epoch equals the first Trainer's next epoch
    te = GraphDataset(files[1], train_source=path, clustering_method="mcl")
    mem2 = MemoryOutputExporter()
    t2 = Trainer(FoutNet, dataset_test=te, pretrained_model=path, cuda=True, output_exporters=[mem2])
    t2.dataset_train, t2.dataset_val = _sets(*files)
    t2.train(nepoch=1, batch_size=8, shuffle=False, validate=True, best_model=False, filename=None)
    assert t2._fused and t2._fused.optimizer == "adamax" and t2._fused.loss == "huber"  # noqa: SLF001
    assert int(t2._fused.counter[0].item()) == 12  # noqa: SLF001
    mem.records.clear()
    t.train(nepoch=1, batch_size=8, shuffle=False, validate=True, best_model=False, filename=None)
    np.testing.assert_allclose(_losses(mem2, "training"), _losses(mem, "training"), rtol=1e-6)
    for k, v in t.model.state_dict().items():
        np.testing.assert_allclose(t2.model.state_dict()[k].cpu().numpy(), v.cpu().numpy(), rtol=1e-6, atol=1e-8, err_msg=k)


def test_trainer_adam_with_decoupled_decay_runs_the_adamw_rule(files):
    """torch.optim.Adam(decoupled_weight_decay=True) assigned to the Trainer
    used to pass the Adam check and run with L2 decay."""
    tr, va = _sets(*files)
    t = Trainer(fout_amd.FoutNet, tr, va, cuda=True, output_exporters=[MemoryOutputExporter()], precluster=False)
    t.optimizer = torch.optim.Adam(t.model.parameters(), lr=1e-3, weight_decay=1e-2, decoupled_weight_decay=True)
    t._fused = None  # noqa: SLF001
    step = t._fused_step()  # noqa: SLF001
    assert step is not None and step.optimizer == "adamw" and step.weight_decay == 1e-2


# ---------------------------------------------------- 5. captured against loop
@pytest.mark.parametrize("model_cls", [fout_amd.FoutNet, ginet_amd.GINet])
def test_captured_epochs_bit_identical_adamw_smooth_l1(files, model_cls):
    from deeprank2_amd import trainer as trainer_mod

    res = []
    for captured in (True, False):
        tr, va = _sets(*files)
        mem = MemoryOutputExporter()
        torch.manual_seed(21)
        trainer_mod.Trainer.capture_epochs = captured
        try:
            t = Trainer(model_cls, tr, va, cuda=True, output_exporters=[mem], precluster=False)
            t.configure_optimizers(torch.optim.AdamW, lr=1e-3, weight_decay=1e-2)
            t.set_lossfunction(nn.SmoothL1Loss)
            t.train(nepoch=3, batch_size=5, shuffle=True, validate=True, best_model=False, filename=None)
        finally:
            trainer_mod.Trainer.capture_epochs = True
        assert t._fused and t._fused.optimizer == "adamw" and t._fused.loss == "smooth_l1"  # noqa: SLF001
        assert bool(t._runners) == captured  # noqa: SLF001  (the captured path ran)
        res.append((mem.records, {k: v.detach().cpu() for k, v in t.model.state_dict().items()}))
    (ra, pa), (rb, pb) = res
    assert [r["loss"] for r in ra] == [r["loss"] for r in rb]
    assert [r["output"] for r in ra] == [r["output"] for r in rb]
    for k in pa:
        assert torch.equal(pa[k], pb[k]), k


# -------------------------------------------------- 6. gradients-supplied update
def test_adamax_after_allreduce_matches_the_single_process_step(tmp_path):
    """Data-parallel path on a one-rank gloo group: the reduce launch only
    writes gradients (enabled == 0), the all-reduce runs, and the update
    launch reads them back (slab == NULL)."""
    import torch.distributed as dist

    datas = _datas("foutnet", 6, 11)
    model_o = _oracle_model("foutnet", 9)
    h = BatchHandle(_store("foutnet", datas), np.arange(6))
    solo = FusedTrainStep(_gpu_model("foutnet", model_o), lr=1e-3, weight_decay=1e-2, optimizer="adamax", loss="huber", loss_param=0.5)
    for _ in range(3):
        l_solo, _ = solo.step(h)
    l_solo = l_solo.clone()
    store = dist.FileStore(str(tmp_path / "pg_store"), 1)
    dist.init_process_group("gloo", store=store, rank=0, world_size=1)
    try:
        ddp = FusedTrainStep(_gpu_model("foutnet", model_o), lr=1e-3, weight_decay=1e-2, optimizer="adamax", loss="huber", loss_param=0.5, process_group=dist.group.WORLD)
        for _ in range(3):
            l_ddp, _ = ddp.step(h)
        torch.cuda.synchronize()
    finally:
        dist.destroy_process_group()
    assert int(ddp.counter[0].item()) == 3
    np.testing.assert_allclose(l_ddp.cpu().numpy(), l_solo.cpu().numpy(), rtol=1e-6)
    for n, a, b, (ma, ua), (mb, ub) in zip(fout_amd.PARAM_NAMES, ddp.params, solo.params, ddp.states, solo.states):
        np.testing.assert_allclose(a.detach().cpu().numpy(), b.detach().cpu().numpy(), err_msg=n, **UPD)
        np.testing.assert_allclose(ma.cpu().numpy(), mb.cpu().numpy(), err_msg=n, **UPD)
        np.testing.assert_allclose(ua.cpu().numpy(), ub.cpu().numpy(), err_msg=n, **UPD)


# ------------------------------------------------ 7. the reduce launch on its own
# A synthetic table through ctypes, no model.  (numel, kind, off1, off2, cols):
# numel 1 / 65 / 512 give a block a partial, a straddling and a full 64-element
# tile; every recipe kind occurs, OUTER with 64 columns.
_Z, _SLAB, _OUTER, _HEAD = _lib.DR_GRAD_ZERO, _lib.DR_GRAD_SLAB, _lib.DR_GRAD_OUTER, _lib.DR_GRAD_HEAD
RT_PARAMS = [
    (65, _SLAB, 0, 0, 0), (1, _Z, 0, 0, 0), (512, _OUTER, 0, 8, 64), (1, _HEAD, 72, 0, 0),
    (512, _SLAB, 65, 0, 0), (65, _HEAD, 73, 0, 0), (65, _OUTER, 0, 8, 64), (65, _Z, 0, 0, 0),
]  # fmt: skip
RT_SLAB_STRIDE, RT_HEAD_STRIDE = 580, 140
# (n_batch, slab_rows): chunks of fewer than 8 rows and empty ones; the
# 24-row tail loop; 270 slab rows, more than one 24-row group per chunk
RT_BATCHES = [(5, 1), (70, 1), (90, 3)]
RT_ADAM = dict(lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=1e-2)


def _rt_columns_fit():
    for n, kind, o1, o2, cols in RT_PARAMS:
        if kind == _SLAB:
            assert o1 + n <= RT_SLAB_STRIDE
        elif kind == _HEAD:
            assert o1 + n <= RT_HEAD_STRIDE
        elif kind == _OUTER:
            assert o1 + (n + cols - 1) // cols <= RT_HEAD_STRIDE and o2 + cols <= RT_HEAD_STRIDE


@functools.lru_cache(maxsize=None)
def _rt_partials(n_batch, slab_rows):
    """Seeded per-graph partials on the host: slab rows, head rows, loss terms."""
    g = torch.Generator().manual_seed(1000 * n_batch + slab_rows)
    slab = torch.randn(n_batch * slab_rows, RT_SLAB_STRIDE, generator=g)
    head = torch.randn(n_batch, RT_HEAD_STRIDE, generator=g)
    return slab, head, torch.rand(n_batch, generator=g)


class ReduceState:
    """Device buffers one reduce run owns (the same seeded start for every
    run): parameters, moments, gradients, step counter, loss, fault flag."""

    def __init__(self):
        g = torch.Generator().manual_seed(5)
        numel = [p[0] for p in RT_PARAMS]
        self.p = [torch.randn(n, generator=g).to(DEV) for n in numel]
        self.m = [(0.1 * torch.randn(n, generator=g)).to(DEV) for n in numel]
        self.v = [(0.01 * torch.rand(n, generator=g)).to(DEV) for n in numel]
        self.g = [torch.randn(n, generator=g).to(DEV) for n in numel]
        self.counter = torch.zeros(2, dtype=torch.int64, device=DEV)
        self.loss = torch.full((1,), 8.0, device=DEV)
        self.fault = torch.zeros(1, dtype=torch.int32, device=DEV)
        self.div = torch.full((1,), 4.0, device=DEV)

    def table(self, slab_rows):
        t = _lib.ParamTableC()
        for i, (n, kind, o1, o2, cols) in enumerate(RT_PARAMS):
            t.param[i], t.grad[i] = self.p[i].data_ptr(), self.g[i].data_ptr()
            t.exp_avg[i], t.exp_avg_sq[i] = self.m[i].data_ptr(), self.v[i].data_ptr()
            t.numel[i] = n
            t.recipe[i] = _lib.GradRecipeC(kind, o1, o2, cols)
        t.n_params, t.slab_stride, t.head_stride, t.slab_rows = len(RT_PARAMS), RT_SLAB_STRIDE, RT_HEAD_STRIDE, slab_rows
        return t

    def adam(self, grad_div=False):
        a = _lib.AdamC()
        a.lr, a.beta1, a.beta2, a.eps, a.weight_decay = (RT_ADAM[k] for k in ("lr", "beta1", "beta2", "eps", "weight_decay"))
        a.enabled = 1
        a.step_counter, a.fault = self.counter.data_ptr(), self.fault.data_ptr()
        if grad_div:
            a.grad_div = self.div.data_ptr()
        return a

    def host(self):
        torch.cuda.synchronize()
        cat = lambda ts: torch.cat([t.cpu() for t in ts])  # noqa: E731
        return {"param": cat(self.p), "exp_avg": cat(self.m), "exp_avg_sq": cat(self.v), "grad": cat(self.g), "loss": self.loss.cpu(), "counter": self.counter.cpu()}


def reduce_call(lib, entry, kind, table, slab, head, n_batch, adam, lpg, scale, loss):
    """One reduce launch on the current stream.  entry: "adam" =
    dr_reduce_update; "opt" / "opt_om" = dr_reduce_update_opt with om_beta* 0 /
    fl(1 - beta) rounded from double."""
    stream = _lib.stream_ptr(torch.device(DEV))
    if entry == "adam":
        assert kind == _lib.DR_OPT_ADAM
        rc = lib.dr_reduce_update(ctypes.byref(table), _lib.ptr(slab), _lib.ptr(head), n_batch, ctypes.byref(adam), _lib.ptr(lpg), scale, _lib.ptr(loss), stream)
    else:
        om = (0.0, 0.0) if entry == "opt" else (1.0 - RT_ADAM["beta1"], 1.0 - RT_ADAM["beta2"])
        opt = _lib.OptimC(adam, kind, *om, 0)
        rc = lib.dr_reduce_update_opt(ctypes.byref(table), _lib.ptr(slab), _lib.ptr(head), n_batch, ctypes.byref(opt), _lib.ptr(lpg), scale, _lib.ptr(loss), stream)
    assert rc == 0, (entry, kind, rc)


def reduce_three_steps(lib, entry, kind, n_batch, slab_rows):
    """Three steps from the seeded start on the (n_batch, slab_rows) partials,
    the step number taken from the device counter: every output, on the host."""
    _rt_columns_fit()
    slab, head, lpg = (x.to(DEV) for x in _rt_partials(n_batch, slab_rows))
    st = ReduceState()
    table, adam = st.table(slab_rows), st.adam()
    for _ in range(3):
        st.counter[1].copy_(st.counter[0])  # the snapshot a graph pass takes
        reduce_call(lib, entry, kind, table, slab, head, n_batch, adam, lpg, 1.0 / n_batch, st.loss)
    return st.host()


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


@pytest.mark.parametrize(("n_batch", "slab_rows"), RT_BATCHES)
def test_reduce_launch_adam_entries_agree_and_sum_within_the_fp32_bound(n_batch, slab_rows):
    lib = _lib.load()
    ref = reduce_three_steps(lib, "adam", _lib.DR_OPT_ADAM, n_batch, slab_rows)
    for entry in ("opt", "opt_om"):  # the Adam kernel forms 1.f - beta itself, whatever om_beta* holds
        out = reduce_three_steps(lib, entry, _lib.DR_OPT_ADAM, n_batch, slab_rows)
        for k, v in ref.items():
            assert torch.equal(_bits(out[k]), _bits(v)), (entry, k)
    assert ref["counter"][0] == 3
    start = ReduceState().host()
    assert not torch.equal(ref["param"], start["param"])
    # each gradient against a float64 sum of the same partials: fp32 recursive
    # summation of nb terms is within nb * 2^-24 * sum|terms| of the exact sum
    slab, head, lpg = (x.double() for x in _rt_partials(n_batch, slab_rows))
    u, lo = 2.0**-24, 0
    for n, kind, o1, o2, cols in RT_PARAMS:
        got = ref["grad"][lo : lo + n].double()
        lo += n
        if kind == _Z:
            assert not got.any()
            continue
        if kind == _SLAB:
            terms = slab[:, o1 : o1 + n]
        elif kind == _HEAD:
            terms = head[:, o1 : o1 + n]
        else:
            e = torch.arange(n)
            terms = head[:, o1 + e // cols] * head[:, o2 + e % cols]
        bound = terms.shape[0] * u * terms.abs().sum(0)
        err = (got - terms.sum(0)).abs()
        print(f"reduce n_batch={n_batch} slab_rows={slab_rows} kind={kind} numel={n}: max err/bound {float((err / bound).max()):.3g}")
        assert (err <= bound).all(), (kind, n)
    scale = 1.0 / n_batch  # the loss: n_batch - 1 additions and the scaling
    assert abs(float(ref["loss"]) - float(lpg.sum()) * scale) <= (n_batch + 1) * u * float(lpg.abs().sum()) * scale


def test_reduce_launch_divides_supplied_gradients_and_loss():
    """slab == head == NULL with grad_div: the gradients in the table and the
    loss already in loss_out are divided (by 4: exact), then the update runs.
    Three steps."""
    st = ReduceState()
    start = st.host()
    table, adam = st.table(1), st.adam(grad_div=True)
    for _ in range(3):
        st.counter[1].copy_(st.counter[0])
        reduce_call(_lib.load(), "opt", _lib.DR_OPT_ADAM, table, None, None, 0, adam, None, 1.0, st.loss)
    out = st.host()
    assert torch.equal(out["grad"], start["grad"] / 64.0)  # three launches, each divides what it finds
    assert float(out["loss"]) == float(start["loss"]) / 64.0
    assert out["counter"][0] == 3 and not torch.equal(out["param"], start["param"])


def test_reduce_launch_with_fault_flag_reports_nan_and_keeps_state():
    """*fault = 1 (the flag a graph pass sets when it gives up a hand-off; a
    value, not a device fault): NaN loss and gradients, nothing updated."""
    n_batch, slab_rows = RT_BATCHES[1]
    slab, head, lpg = (x.to(DEV) for x in _rt_partials(n_batch, slab_rows))
    st = ReduceState()
    start = st.host()
    st.fault.fill_(1)
    table, adam = st.table(slab_rows), st.adam()
    for _ in range(3):
        st.counter[1].copy_(st.counter[0])
        reduce_call(_lib.load(), "opt", _lib.DR_OPT_ADAM, table, slab, head, n_batch, adam, lpg, 1.0 / n_batch, st.loss)
    out = st.host()
    assert torch.isnan(out["loss"]).all() and torch.isnan(out["grad"]).all()
    for k in ("param", "exp_avg", "exp_avg_sq"):
        assert torch.equal(out[k], start[k]), k
    assert out["counter"][0] == 0
