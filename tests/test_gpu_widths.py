"""FoutNet, SGAT, ginet_nocluster and GINet at the node-feature widths F and
output counts OUT on which their kernels branch (``width_cases.py``), every
case against one **fp64** training step of the CPU oracle.

The other whole-model tests run F = 30 and F = 50 (both 2 mod 4) and at most
3 outputs.  Here, per family (``test_width_cases_host.py`` asserts that these
cases take each value):

* FoutNet / SGAT per-graph kernel: the fused front with chunks to drop
  (F = 1, 4, 8: ``nch`` 1, 1, 2) and without (29, 32); the other branch with
  idle lanes (F = 8 with K0 = 70, ``k0_over_64``), with a second round (33)
  and full (64); K without padding rows (8, 32, 64) and with 14 of 16
  (F = 1); the ``x | Zm`` seam of the MFMA k-groups at F % 4 = 0 and 1; the
  weight image up to its last register slot (64, 14: 6,142 of 6,144 words);
  16 outputs through fc2, ``dout16`` and the cross entropy.
* FoutNet / SGAT tile + tail path: the same widths with and without halos.
* ginet_nocluster: per-graph kernel and tile pipeline at KP = 16, 32, 48, 64.
* GINet per-graph pass: F = 32 | 33 (the K = 32 | 64 switch), 1 and 64, with
  and without the store's Z array, which must agree bit for bit; the same
  widths through its fp32 tile + tail path; and the K0 = 70 batch.

Tolerances are the suite's: outputs rtol = atol = 1e-4, loss 1e-4 relative,
gradients ``_util.assert_grad_close`` (ntol 1e-5 on ginet_nocluster's tile
pipeline), Adam against ``torch.optim.Adam`` fed the kernel's gradients at
rtol 1e-5 / atol 1e-7.  Each case prints its largest error as a fraction of
that tolerance (``pytest -s``).

Measured on an MI355X: every case within 0.051 of its tolerance (GINet at
(64, 16), fc2.weight; FoutNet at most 0.013, SGAT 0.036, ginet_nocluster
0.029), the level of the fp32 oracle's own distance from the fp64 one.  Before
the fix to fout_graph_kernel's depth-0 pooling for K0 > 64 (its staging arrays
hold 1,024 pairs, K0 = 70 has 1,120) the ``k0_over_64`` case gave the right
outputs and loss and conv1 gradients 1,000 (FoutNet) and 1,860 (SGAT) times
the tolerance off.

The tile + tail path takes at most 64 depth-0 clusters, so ``k0_over_64``
cannot run forced through it: ``test_k0_over_64_forced_large_is_refused``
holds that the refusal comes before any launch.
"""

from __future__ import annotations

import functools

import numpy as np
import pytest
import torch
import width_cases as W
from _util import assert_grad_close

import graph_zoo
from deeprank2_amd import _lib
from deeprank2_amd.engine import FusedTrainStep
from deeprank2_amd.fused import LDS_MAX, BatchHandle, lds_for
from deeprank2_amd.neuralnets.gnn import foutnet, ginet, ginet_nocluster, sgat
from deeprank2_amd.store import GraphStore, pack_graphs, records_from_batch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = dict(rtol=1e-4, atol=1e-4)

# family -> (module, model class, plan kind of the large path)
MODELS = {
    "foutnet": (foutnet, foutnet.FoutNet, "fout"),
    "sgat": (sgat, sgat.SGAT, "sgat"),
    "nocluster": (ginet_nocluster, ginet_nocluster.GINet, None),
    "ginet": (ginet, ginet.GINet, "ginet"),
}
PATHS = {"per_graph": dict(force_large=False), "large": dict(force_large=True, large_halos=True), "large_hbm_gather": dict(force_large=True, large_halos=False)}
FOUT = ("foutnet", "sgat")


def _id(v):
    return f"F{v[0]}-OUT{v[1]}" if isinstance(v, tuple) else str(v)


@functools.lru_cache(maxsize=None)
def _store(family, f, out, batch):
    return GraphStore(W.packed(family, f, out, batch), DEV)


def _handle(family, f, out, batch, store=None, **knobs):
    h = BatchHandle(_store(family, f, out, batch) if store is None else store, np.arange(len(W.datas(family, f, out, batch))))
    for k, v in knobs.items():
        setattr(h, k, v)
    return h


def _model(family, c):
    m = MODELS[family][1](c["f"], c["out_dim"], W.FAMILIES[family][1])
    m.load_state_dict(c["state"])
    return m.to(DEV).train()


def _assert_path(family, h, out_dim, force_large, halos=True):
    """The launch took the kernels the case is about."""
    mod, _, kind = MODELS[family]
    assert lds_for(mod.SPEC, h, out_dim) <= LDS_MAX  # small graphs: the large path only when forced
    plan = h._lds.get("nc_plan") if kind is None else h._lds.get(("large", out_dim, False, kind))  # noqa: SLF001
    assert (plan is not None) == force_large
    if force_large and kind is not None:
        assert (plan.halo_tensors is not None) == halos


def _train_step(family, f, out, batch="asym", store=None, **knobs):
    """One ``FusedTrainStep.step`` from the case's parameters (fixed dropout
    mask where the model has dropout): the comparison record, the step object
    and the parameters before the step."""
    c = W.case(family, f, out, batch)
    h = _handle(family, f, out, batch, store=store, **knobs)
    assert not h.store.packed.transpose_aliased and h.store.n_feat == f
    step = FusedTrainStep(_model(family, c), loss=c["loss_kind"])
    step.acc = False
    before = [p.detach().clone() for p in step.params]
    loss, res = step.step(h, mask=None if c["mask"] is None else c["mask"].to(torch.uint8).to(DEV))
    torch.cuda.synchronize()
    _assert_path(family, h, out, knobs.get("force_large", False), knobs.get("large_halos", True))
    names = MODELS[family][0].PARAM_NAMES
    got = {"out": res.cpu().numpy().copy(), "loss": float(loss), "grads": {n: g.cpu().numpy().copy() for n, g in zip(names, step.grads)}}
    return got, step, before


def _check_vs_fp64(family, f, out, batch="asym", **knobs):
    got, step, before = _train_step(family, f, out, batch, **knobs)
    ref = W.case(family, f, out, batch)
    ntol = W.grad_ntol(family, knobs.get("force_large", False))
    assert set(got["grads"]) == set(ref["grads"])
    r = W.ratios(got, ref, ntol=ntol)
    worst = max(r, key=r.get)
    label = {k: v for k, v in knobs.items() if k != "store"} | ({"use_agg_x": knobs["store"].use_agg_x} if "store" in knobs else {})
    print(f"[widths {family} F={f} OUT={out} {batch} {label}] worst {worst}: {r[worst]:.3f} of the tolerance; out {r['out']:.3f} loss {r['loss']:.3f}")
    assert got["out"].shape == ref["out"].shape
    np.testing.assert_allclose(got["out"], ref["out"], **TOL)
    assert got["loss"] == pytest.approx(ref["loss"], rel=1e-4)
    for n, g in ref["grads"].items():
        if W.is_zero_grad(family, n):
            assert not np.any(got["grads"][n]), f"{n}: expected exact zeros"
        else:
            assert_grad_close(got["grads"][n], g, ntol=ntol, err_msg=n)
    # the fused Adam against torch.optim.Adam fed the same (kernel) gradients
    opt = [torch.nn.Parameter(b) for b in before]
    for o, g in zip(opt, step.grads):
        o.grad = g.detach().clone()
    torch.optim.Adam(opt, lr=1e-3, weight_decay=1e-5).step()
    for n, o, p in zip(MODELS[family][0].PARAM_NAMES, opt, step.params):
        np.testing.assert_allclose(p.detach().cpu().numpy(), o.detach().cpu().numpy(), rtol=1e-5, atol=1e-7, err_msg=n)
    return got


# --------------------------------------------------------------------------
# FoutNet, SGAT
# --------------------------------------------------------------------------


@pytest.mark.parametrize("path", ["per_graph", "large"])
@pytest.mark.parametrize("width", W.FOUT_WIDTHS, ids=_id)
@pytest.mark.parametrize("family", FOUT)
def test_fout_sgat_widths_vs_fp64_oracle(family, width, path):
    """fout_graph_kernel, and dr_fout_large_pass / dr_sgat_large_pass with LDS halos."""
    _check_vs_fp64(family, *width, **PATHS[path])


@pytest.mark.parametrize("width", [(29, 5), (33, 16)], ids=_id)
@pytest.mark.parametrize("family", FOUT)
def test_fout_sgat_large_path_hbm_gather_vs_fp64_oracle(family, width):
    """The tile kernel's per-edge gather from HBM (``large_halos = False``)."""
    _check_vs_fp64(family, *width, **PATHS["large_hbm_gather"])


@pytest.mark.parametrize("family", W.K0_FAMILIES)
def test_k0_over_64_per_graph_vs_fp64_oracle(family):
    """r4(F) = 8 with K0 = 70 in the batch.  FoutNet / SGAT: the branch without
    the fused front at ``nch`` = 2, six of every row group's eight lanes idle,
    and more (cluster, channel) pairs than the workgroup has threads.  GINet:
    K0 * 32 keys and pooled rows, past two rounds of the workgroup."""
    _check_vs_fp64(family, *W.K0_OVER_64, batch="k0_over_64", **PATHS["per_graph"])


def _assert_untouched(step, before, counter):
    torch.cuda.synchronize()
    for n, p, b in zip(step.spec.param_names, step.params, before):
        assert torch.equal(p, b), n
    for m, v in step.states:
        assert not m.any() and not v.any()
    assert torch.equal(step.counter, counter) and step.step_count == 0


def _refused(family, f, out, match, datas=None, use_agg_x=None, **knobs):
    """A step the entry point must refuse: RuntimeError, with the parameters,
    the optimizer state and the step counters as they were."""
    fe = W.FAMILIES[family][1]
    if datas is None:
        datas = graph_zoo.resized(graph_zoo.asymmetric(fe=fe, **{**graph_zoo.ASYM_BATCH, "n": 2}), f, fe)
    store = GraphStore(pack_graphs(records_from_batch(graph_zoo.batch(datas)), require_clusters=family != "nocluster"), DEV)
    if use_agg_x is not None:
        store.use_agg_x = use_agg_x
    h = BatchHandle(store, np.arange(len(datas)))
    for k, v in knobs.items():
        setattr(h, k, v)
    torch.manual_seed(11)
    step = FusedTrainStep(MODELS[family][1](f, out, fe).to(DEV).train(), loss="mse" if out == 1 else "ce")
    step.acc = False
    before = [p.detach().clone() for p in step.params]
    counter = step.counter.clone()
    mask = torch.ones(len(datas), 128, dtype=torch.uint8, device=DEV) if W.FAMILIES[family][2] else None
    with pytest.raises(RuntimeError, match=match):
        step.step(h, mask=mask)
    _assert_untouched(step, before, counter)


@pytest.mark.parametrize("family", W.K0_FAMILIES)
def test_k0_over_64_forced_large_is_refused(family):
    """The tile + tail path combines the depth-0 maxima of at most 64 clusters
    per graph (dr_large_plan.k0_max): the plan refuses this batch on the host,
    before any launch, and the step changes nothing."""
    f, out = W.K0_OVER_64
    _refused(family, f, out, r"70 depth-0 clusters \(> 64\)", datas=W.datas(family, f, out, "k0_over_64"), **PATHS["large"])


# --------------------------------------------------------------------------
# ginet_nocluster, GINet
# --------------------------------------------------------------------------


@pytest.mark.parametrize("path", ["per_graph", "large"])
@pytest.mark.parametrize("width", W.WIDTHS["nocluster"], ids=_id)
def test_nocluster_widths_vs_fp64_oracle(width, path):
    """dr_ginet_nocluster_graph_pass in training mode, and the tile pipeline
    dr_ginet_nocluster_large_pass (KP = r16(F), its padded weight and Z rows,
    the 2 KP / 16 dW1 tiles)."""
    _check_vs_fp64("nocluster", *width, force_large=path == "large")


@pytest.mark.parametrize("width", W.WIDTHS["ginet"], ids=_id)
def test_ginet_per_graph_widths_vs_fp64_oracle(width):
    """The per-graph training pass staged from the store's records and Z = A x
    (``use_agg_x``), and gathering in the kernel: both against the oracle, and
    bit-identical to each other."""
    f, out = width
    runs = []
    for use_z in (True, False):
        store = GraphStore(W.packed("ginet", f, out, "asym"), DEV)
        store.use_agg_x = use_z
        runs.append(_check_vs_fp64("ginet", f, out, store=store))
        assert (store._agg_x is not None) == use_z  # noqa: SLF001  (the entry taken)
    a, b = runs
    assert np.array_equal(a["out"], b["out"]) and a["loss"] == b["loss"]
    for n in ginet.PARAM_NAMES:
        assert np.array_equal(a["grads"][n], b["grads"][n]), n


@pytest.mark.parametrize("halos", [True, False], ids=["halos", "hbm_gather"])
@pytest.mark.parametrize("width", W.WIDTHS["ginet"], ids=_id)
def test_ginet_large_path_widths_vs_fp64_oracle(width, halos):
    """dr_ginet_large_pass in fp32 (tile conv1 kernel + per-graph tail), which
    test_gpu_large.py and test_gpu_topology.py run at F = 30 (the fp32 control
    of test_gpu_bf16_parity.py takes the per-graph pass): KP = r16(F) = 16, 32,
    48, 64 with and without LDS halos."""
    _check_vs_fp64("ginet", *width, force_large=True, large_halos=halos)


# --------------------------------------------------------------------------
# tile + tail path against the single-workgroup kernel, bit for bit
# --------------------------------------------------------------------------


@pytest.mark.parametrize("width", [(29, 5), (32, 1), (8, 16), (33, 16), (64, 14)], ids=_id)
@pytest.mark.parametrize("family", FOUT)
def test_large_path_bit_identical_to_single_workgroup_kernel(family, width):
    """test_gpu_fout_large.py's assertion at other widths: outputs, slab, head
    and per-graph loss of one FORWARD | BACKWARD pass are equal bit for bit
    between the per-graph kernel and the tile + tail path with and without
    halos.  (33, 16) and (64, 14) are kept in: both paths sum a row's
    neighbours in CSR order and run the same MFMA k-loop over KP = r16(2F),
    and nothing on the host side says otherwise (the carves agree on XS and KP,
    test_width_cases_host.py)."""
    f, out = width
    c = W.case(family, f, out)
    mod = MODELS[family][0]
    params = _model(family, c).ordered_params()
    b = len(c["datas"])
    res = []
    for path in ("per_graph", "large", "large_hbm_gather"):
        h = _handle(family, f, out, "asym", **PATHS[path])
        res_out = torch.empty(b, out, device=DEV)
        slab = torch.empty(b * mod.SPEC.slab_stride(f), device=DEV)
        head = torch.zeros(b * mod.SPEC.head_stride(out), device=DEV)
        lpg = torch.empty(b, device=DEV)
        kind = _lib.DR_LOSS_MSE if out == 1 else _lib.DR_LOSS_CE
        mod.graph_pass(h, params, out, _lib.DR_PASS_FORWARD | _lib.DR_PASS_BACKWARD, loss_kind=kind, loss_scale=1 / b, out=res_out, loss_per_graph=lpg, slab=slab, head=head)
        torch.cuda.synchronize()
        _assert_path(family, h, out, PATHS[path]["force_large"], PATHS[path].get("large_halos", True))
        res.append((res_out.cpu(), slab.cpu(), head.cpu(), lpg.cpu()))
    assert all(torch.isfinite(t).all() for t in res[0])
    np.testing.assert_allclose(res[0][0].numpy(), c["out"], **TOL)  # (the pass compared is the one the oracle checks)
    for k, other in enumerate(res[1:]):
        for what, x, y in zip(("out", "slab", "head", "loss"), res[0], other):
            assert torch.equal(x, y), f"{('halos', 'hbm gather')[k]}: {what}"


# --------------------------------------------------------------------------
# refusals: argument checks that return before any launch
# --------------------------------------------------------------------------


def test_foutnet_per_graph_refuses_a_weight_image_past_its_registers():
    """32 F + 3184 + 65 OUT > 6144: (64, 15) is one output past the last
    register slot (64, 14 runs above), (91, 1) the first F past it."""
    assert W.image_words(64, 15) > 6144 and W.image_words(91, 1) > 6144  # noqa: PLR2004
    _refused("foutnet", 64, 15, "dr_fout_graph_pass failed")
    _refused("foutnet", 91, 1, "dr_fout_graph_pass failed")


def test_foutnet_large_path_refuses_65_features():
    _refused("foutnet", 65, 1, "dr_fout_large_pass failed", **PATHS["large"])


@pytest.mark.parametrize("use_agg_x", [False, True], ids=["gather", "records"])
def test_ginet_refuses_65_features(use_agg_x):
    """The gather entry, and the record entry: the store builds its Z = A x
    rows and records at any width (``dr_aggregate_x`` takes any stride >= F),
    the pass that would read them refuses."""
    _refused("ginet", 65, 1, "dr_ginet_graph_pass(_rec)? failed", use_agg_x=use_agg_x)
