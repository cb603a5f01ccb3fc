"""The references of ``test_gpu_multi_output_mse.py``, on the CPU.

The project's regression losses with more than one output read column 0 of the
outputs and take the factor 1 / (B * OUT) (``engine._layered_step``,
``engine.loss_scale``).  ``width_cases.oracle(..., loss="mse")`` restates that on
the family's fp64 oracle forward; here, for every case of
``width_cases.MSE_MULTI`` (VanillaNetwork's cases: test_vanilla_zoo_host.py):

* the loss is that formula on the oracle's own outputs and the stored targets
  (regression targets, not the class indices of the cross-entropy cases);
* the last linear layer's gradient rows, and bias entries, from 1 on are
  exactly zero, in fp64 and in fp32, and row 0 is not: a head that lets the
  other logits into its backward cannot match this reference;
* every other gradient is live, and what would reach them through rows 1.. of
  fc2 is far beyond the GPU comparison's tolerance: the same oracle with
  ``dout[1..] = out[:, 1..]`` (the defect the GPU test was written for) misses
  by more than 100 times the tolerance;
* the fp32 oracle stays within a tenth of the GPU comparison's tolerance of
  the fp64 one (``test_width_cases_host.py``'s condition on the inputs).
"""

from __future__ import annotations

import numpy as np
import pytest
import torch
import width_cases as W

HEADROOM = 0.1
CASES = [(fam, f, out) for fam, ws in W.MSE_MULTI.items() for f, out in ws]
IDS = lambda c: f"{c[0]}-F{c[1]}-OUT{c[2]}"  # noqa: E731


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_reference_is_column_0_over_b_times_out(c):
    family, f, out = c
    ref = W.oracle(family, f, out, loss="mse")
    ds = W.datas(family, f, out, loss="mse")
    y = np.array([float(d.y) for d in ds])
    assert ref["out"].shape == (len(ds), out) and out > 1
    assert not np.array_equal(y, np.arange(len(ds)) % out)  # the stored regression targets
    assert ref["loss"] == pytest.approx(float(((ref["out"][:, 0] - y) ** 2).sum() / (len(ds) * out)), rel=1e-12)
    assert (ref["mask"] is not None) == W.FAMILIES[family][2]
    # the cross-entropy case of the same (F, OUT) is untouched by the override
    assert W.case(family, f, out)["loss_kind"] == "ce" and W.case(family, f, out, loss="mse")["loss_kind"] == "mse"
    np.testing.assert_array_equal([float(d.y) for d in W.datas(family, f, out)], np.arange(len(ds)) % out)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_rows_from_1_on_are_exactly_zero(c, dtype):
    family, f, out = c
    g = W.oracle(family, f, out, dtype=dtype, loss="mse")["grads"]
    assert g["fc2.weight"].shape[0] == out == g["fc2.bias"].shape[0]
    assert not np.any(g["fc2.weight"][1:]) and not np.any(g["fc2.bias"][1:])
    assert np.any(g["fc2.weight"][0]) and g["fc2.bias"][0] != 0
    for n, v in g.items():
        assert np.isfinite(v).all(), n
        assert np.any(v) != W.is_zero_grad(family, n), n


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_fp32_oracle_within_a_tenth_of_the_tolerance(c):
    family, f, out = c
    ref, ref32 = W.oracle(family, f, out, loss="mse"), W.oracle(family, f, out, dtype=torch.float32, loss="mse")
    r = W.ratios(ref32, ref)
    worst = max(r, key=r.get)
    print(f"[headroom mse {IDS(c)}] worst {worst} {r[worst]:.4f}")
    assert r[worst] <= HEADROOM, r


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_logits_left_in_dout_would_be_far_outside_the_tolerance(c):
    """The gradient of ``loss + sum_b sum_{q >= 1} out[b, q]^2 / 2`` is what a
    head computes that leaves the logits 1.. in ``dout``: against the
    reference it misses fc2's rows 1.., and some earlier layer's gradient, by
    more than 100 times what the GPU comparison allows."""
    family, f, out = c
    cls, fe, has_drop = W.FAMILIES[family]
    ref = W.oracle(family, f, out, loss="mse")
    from _util import fixed_dropout

    import graph_zoo

    ds = W.datas(family, f, out, loss="mse")
    model = cls(f, out, fe).train()
    model.load_state_dict(ref["state"])
    if has_drop:
        model.dropout_fn = fixed_dropout(ref["mask"].double())
    model = model.double()
    torch.set_default_dtype(torch.float64)
    try:
        bat = graph_zoo.batch(ds)
        for k in ("x", "edge_attr", "pos", "y"):
            setattr(bat, k, getattr(bat, k).double())
        y = bat.y.clone()
        res = model(bat)
        (((res[:, 0] - y) ** 2).sum() / (len(ds) * out) + 0.5 * (res[:, 1:] ** 2).sum()).backward()
    finally:
        torch.set_default_dtype(torch.float32)
    np.testing.assert_allclose(res.detach().numpy(), ref["out"], rtol=0, atol=1e-12)
    bad = {"out": ref["out"], "loss": ref["loss"], "grads": {n: p.grad.numpy() for n, p in model.named_parameters()}}
    r = W.ratios(bad, ref)
    assert r["fc2.weight"] > 100.0 and r["fc2.bias"] > 100.0, r  # noqa: PLR2004
    assert max(v for n, v in r.items() if not n.startswith("fc2") and n not in ("out", "loss")) > 100.0, r  # noqa: PLR2004
