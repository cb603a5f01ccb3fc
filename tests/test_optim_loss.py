"""Host side of the AdamW / Adamax update rules and the L1 / SmoothL1 / Huber
losses of the fused training step: which torch configurations the Trainer
hands to the kernels (``trainer.fused_config``), the argument checks every
graph-pass entry and ``dr_reduce_update_opt`` make before their first device
call, and the optimizer state dicts (``engine.build_optimizer_state_dict`` /
``read_optimizer_state_dict``).  No GPU needed."""

from __future__ import annotations

import ctypes

import pytest
import torch
from torch import nn

from deeprank2_amd import _lib
from deeprank2_amd.dataset import CLASSIF, REGRESS
from deeprank2_amd.engine import build_optimizer_state_dict, read_optimizer_state_dict
from deeprank2_amd.trainer import fused_config

DR_E_ARG = -1


def _params():
    return [nn.Parameter(torch.zeros(3)), nn.Parameter(torch.zeros(2, 2))]


def test_fused_config_table():
    hyper = {"lr": 2e-3, "weight_decay": 1e-2, "betas": (0.9, 0.999), "eps": 1e-8}
    mse = nn.MSELoss()
    accepted = [
        (torch.optim.Adam(_params(), lr=2e-3, weight_decay=1e-2), "adam"),
        (torch.optim.AdamW(_params(), lr=2e-3, weight_decay=1e-2), "adamw"),
        (torch.optim.Adam(_params(), lr=2e-3, weight_decay=1e-2, decoupled_weight_decay=True), "adamw"),
        (torch.optim.Adamax(_params(), lr=2e-3, weight_decay=1e-2), "adamax"),
    ]
    for opt, kind in accepted:
        assert fused_config(opt, mse, REGRESS) == (kind, hyper, "mse", None, None), type(opt).__name__
    adam = accepted[0][0]
    assert fused_config(adam, nn.HuberLoss(delta=0.3), REGRESS)[2:4] == ("huber", pytest.approx(0.3))
    assert fused_config(adam, nn.SmoothL1Loss(beta=0), REGRESS)[2:4] == ("smooth_l1", 0.0)
    assert fused_config(adam, nn.SmoothL1Loss(), REGRESS)[2:4] == ("smooth_l1", 1.0)
    assert fused_config(adam, nn.L1Loss(), REGRESS)[2:4] == ("l1", None)
    w = torch.tensor([0.25, 0.75])
    cfg = fused_config(accepted[3][0], nn.CrossEntropyLoss(weight=w), CLASSIF)
    assert cfg[0] == "adamax" and cfg[2:4] == ("ce", None) and cfg[4] is w
    rejected = [
        (torch.optim.SGD(_params(), lr=0.01), mse, REGRESS),
        (torch.optim.Adam(_params(), amsgrad=True), mse, REGRESS),
        (torch.optim.AdamW(_params(), amsgrad=True), mse, REGRESS),
        (torch.optim.Adamax(_params(), maximize=True), mse, REGRESS),
        (torch.optim.Adam(_params(), lr=torch.tensor(1e-3)), mse, REGRESS),
        (torch.optim.Adam([{"params": _params()[:1]}, {"params": _params()[1:]}]), mse, REGRESS),
        (adam, nn.MSELoss(reduction="sum"), REGRESS),
        (adam, nn.HuberLoss(reduction="sum"), REGRESS),
        (adam, nn.L1Loss(), CLASSIF),  # a regression loss on a classification task
        (adam, nn.HuberLoss(), CLASSIF),
        (adam, nn.CrossEntropyLoss(), REGRESS),
        (adam, nn.CrossEntropyLoss(label_smoothing=0.1), CLASSIF),
        (adam, nn.NLLLoss(), CLASSIF),
    ]
    for opt, lf, task in rejected:
        assert fused_config(opt, lf, task) is None, (type(opt).__name__, lf, task)


def _pass_calls():
    """Every graph-pass entry as (name, call(pass) -> rc) on structs that are
    never dereferenced: the loss check returns first."""
    lib = _lib.load()
    st = _lib.GraphStoreC()
    st.n_feat, st.x_stride, st.n_edge_feat = 30, 32, 3
    d = ctypes.c_void_p(16)
    gw, fw, vw = _lib.GinetWeightsC(), _lib.FoutWeightsC(), _lib.VanillaWeightsC()
    lp, ncp, vs = _lib.LargePlanC(), _lib.NcPlanC(), _lib.VanillaScratchC()
    s, r = ctypes.byref(st), ctypes.byref
    return [
        ("dr_ginet_graph_pass", lambda p: lib.dr_ginet_graph_pass(s, d, 8, r(gw), r(p), 1024, None)),
        ("dr_ginet_acc_pass", lambda p: lib.dr_ginet_acc_pass(s, d, 8, r(gw), r(p), 1024, 2, None, None, None)),
        ("dr_ginet_large_pass", lambda p: lib.dr_ginet_large_pass(s, d, 8, r(lp), r(gw), r(p), 1024, 1024, None)),
        ("dr_fout_graph_pass", lambda p: lib.dr_fout_graph_pass(s, d, 8, r(fw), r(p), 1024, None)),
        ("dr_sgat_graph_pass", lambda p: lib.dr_sgat_graph_pass(s, d, 8, r(fw), r(p), 1024, None)),
        ("dr_fout_large_pass", lambda p: lib.dr_fout_large_pass(s, d, 8, r(lp), r(fw), r(p), 32, 1024, 1024, None)),
        ("dr_sgat_large_pass", lambda p: lib.dr_sgat_large_pass(s, d, 8, r(lp), r(fw), r(p), 36, 1024, 1024, None)),
        ("dr_ginet_nocluster_graph_pass", lambda p: lib.dr_ginet_nocluster_graph_pass(s, d, 8, r(gw), r(p), 1024, None)),
        ("dr_ginet_nocluster_large_pass", lambda p: lib.dr_ginet_nocluster_large_pass(s, d, 8, r(ncp), r(gw), r(p), None)),
        ("dr_vanilla_graph_pass", lambda p: lib.dr_vanilla_graph_pass(s, d, 8, r(vw), r(p), r(vs), 1024, None)),
        ("dr_vanilla_fused_pass", lambda p: lib.dr_vanilla_fused_pass(s, d, 8, r(vw), r(p), d, d, 1, d, d, 1024, None)),
    ]


@pytest.mark.parametrize(
    ("loss_kind", "loss_param"),
    [
        (6, 1.0),  # an unknown kind (with dout NULL it used to reach the kernel's dout read)
        (-1, 1.0),
        (_lib.DR_LOSS_HUBER, 0.0),
        (_lib.DR_LOSS_HUBER, -0.5),
        (_lib.DR_LOSS_HUBER, float("nan")),
        (_lib.DR_LOSS_HUBER, float("inf")),
        (_lib.DR_LOSS_SMOOTH_L1, -1e-3),
        (_lib.DR_LOSS_SMOOTH_L1, float("nan")),
        (_lib.DR_LOSS_SMOOTH_L1, float("inf")),
    ],
)
def test_graph_pass_entries_refuse_bad_loss_on_the_host(loss_kind, loss_param):
    p = _lib.PassC()
    p.flags = _lib.DR_PASS_FORWARD | _lib.DR_PASS_BACKWARD
    p.out_dim = 1
    p.loss_kind, p.loss_param = loss_kind, loss_param
    for name, call in _pass_calls():
        assert call(p) == DR_E_ARG, name


def test_pass_struct_keeps_its_size_and_names_loss_param():
    names = [f for f, _ in _lib.PassC._fields_]
    assert "loss_param" in names and "pad0" not in names
    assert _lib.PassC.loss_param.offset == _lib.PassC.spin_limit.offset + 4
    assert ctypes.sizeof(_lib.PassC) == 16 + 8 + 16 + 8 + 9 * 8 + 8 + 8 + 8
    assert ctypes.sizeof(_lib.OptimC) == ctypes.sizeof(_lib.AdamC) + 16 and _lib.OptimC.kind.offset == ctypes.sizeof(_lib.AdamC)


def test_reduce_update_opt_refuses_unknown_kind_on_the_host():
    lib = _lib.load()
    table = _lib.ParamTableC()
    table.n_params = 1
    d = ctypes.c_void_p(16)
    for kind in (3, -1):
        opt = _lib.OptimC(_lib.AdamC(), kind)
        assert lib.dr_reduce_update_opt(ctypes.byref(table), d, d, 8, ctypes.byref(opt), None, 1.0, None, None) == DR_E_ARG
    assert lib.dr_reduce_update_opt(ctypes.byref(table), d, d, 8, None, None, 1.0, None, None) == DR_E_ARG
    # a known kind goes on to the table checks every kind shares (param[0] is NULL here)
    for kind in (_lib.DR_OPT_ADAM, _lib.DR_OPT_ADAMW, _lib.DR_OPT_ADAMAX):
        opt = _lib.OptimC(_lib.AdamC(), kind)
        assert lib.dr_reduce_update_opt(ctypes.byref(table), d, d, 8, ctypes.byref(opt), None, 1.0, None, None) == DR_E_ARG


@pytest.mark.parametrize(("kind", "cls", "second"), [("adam", torch.optim.Adam, "exp_avg_sq"), ("adamw", torch.optim.AdamW, "exp_avg_sq"), ("adamax", torch.optim.Adamax, "exp_inf")])
def test_optimizer_state_dict_round_trip(kind, cls, second):
    gen = torch.Generator().manual_seed(3)
    params = _params()
    states = [(torch.randn(p.shape, generator=gen), torch.rand(p.shape, generator=gen)) for p in params]
    hyper = dict(lr=3e-3, betas=(0.8, 0.99), eps=1e-7, weight_decay=1e-3)
    sd = build_optimizer_state_dict(kind, params, states, 7, **hyper)
    opt = cls(params)
    opt.load_state_dict(sd)  # the torch class takes it
    g = opt.param_groups[0]
    assert (g["lr"], tuple(g["betas"]), g["eps"], g["weight_decay"]) == (3e-3, (0.8, 0.99), 1e-7, 1e-3)
    for p, (m, v) in zip(params, states):
        st = opt.state[p]
        assert set(st) == {"step", "exp_avg", second}
        assert float(st["step"]) == 7 and torch.equal(st["exp_avg"], m) and torch.equal(st[second], v)
    back = [(torch.empty_like(m), torch.empty_like(v)) for m, v in states]
    assert read_optimizer_state_dict(kind, opt.state_dict(), back) == (7, 3e-3, (0.8, 0.99), 1e-7, 1e-3)
    for (m, v), (m2, v2) in zip(states, back):
        assert torch.equal(m, m2) and torch.equal(v, v2)
    # before the first step the dict holds no state, and reading it zeroes the moments
    sd0 = build_optimizer_state_dict(kind, params, states, 0, **hyper)
    assert sd0["state"] == {}
    assert read_optimizer_state_dict(kind, sd0, back)[0] == 0
    assert all(not m.any() and not v.any() for m, v in back)


def test_optimizer_state_dict_refuses_another_rule():
    params = _params()
    states = [(torch.zeros_like(p), torch.zeros_like(p)) for p in params]
    adamw = torch.optim.AdamW(params).state_dict()
    adam = torch.optim.Adam(params).state_dict()
    with pytest.raises(ValueError, match="decoupled_weight_decay"):
        read_optimizer_state_dict("adam", adamw, states)  # L2 decay must not be run on an AdamW state
    with pytest.raises(ValueError, match="decoupled_weight_decay"):
        read_optimizer_state_dict("adamw", adam, states)
    with pytest.raises(ValueError, match="amsgrad"):
        read_optimizer_state_dict("adam", torch.optim.Adam(params, amsgrad=True).state_dict(), states)
