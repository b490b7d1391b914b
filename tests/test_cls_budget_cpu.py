"""The budgets of tests/cls_budget.py hold what they should, without a GPU: a torch-fp32 CPU emulation of the tail kernels stays inside
every budget on every case, every planted defect leaves it, the head's conv shapes are accepted by the library's host-side planners and
their CPU emulation is inside the conv budgets, and the golden training step (tests/golden/cls_train_step.npz) has the properties the GPU
comparison relies on."""
import ctypes
import os

import numpy as np
import pytest
import torch

import cls_budget as cb
import train_budget as tb
from conftest import GOLDEN

DTYPES = [torch.bfloat16, torch.float16]


# ------------------------------------------------------------------------------------------------ the budgets are not too tight
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("case", cb.POOL_CASES, ids=cb.pool_id)
def test_pool_emulation_within_budget(case, dtype):
    refs, emu = cb.pool_refs(case, dtype), cb.emulate_pool(cb.pool_inputs(case, dtype), case, dtype)
    print("emulation / allowed", cb.pool_id(case), {k: round(cb.check(emu[k], *refs[k], f"pool {cb.pool_id(case)} {k}", spatial=False), 3) for k in refs})


@pytest.mark.parametrize("case", cb.LIN_CASES, ids=cb.lin_id)
def test_linear_emulation_within_budget(case):
    refs, emu = cb.lin_refs(case), cb.emulate_linear(cb.lin_inputs(case))
    print("emulation / allowed", cb.lin_id(case), {k: round(cb.check(emu[k], *refs[k], f"linear {cb.lin_id(case)} {k}", spatial=False), 3) for k in refs})


def _xent_cases():
    out = [(cb.lin_id(c), cb.xent_logits(c), cb.xent_targets(c)) for c in cb.LIN_CASES]
    z, t, _ = cb.tie_case()
    out.append(("ties", z, t))
    out.append(("out-of-range", *cb.out_of_range_case()))
    return out


@pytest.mark.parametrize("name,z,t", _xent_cases(), ids=[c[0] for c in _xent_cases()])
def test_xent_emulation_within_budget(name, z, t):
    refs = cb.xent_refs(z, t)
    assert cb.xent_mismatches(cb.emulate_xent(z, t), refs, name) == []


def test_tie_and_out_of_range_references():
    z, t, (top1, top5) = cb.tie_case()
    r = cb.xent_refs(z, t)
    assert (r["top1"], r["top5"], r["flags"]) == (top1, top5, 0)
    z, t = cb.out_of_range_case()
    r = cb.xent_refs(z, t)
    assert r["flags"] == 1 and float(r["dlogits"][0][1].abs().max()) == 0.0 and float(r["dlogits"][0][3].abs().max()) == 0.0
    only = cb.xent_refs(z[[0, 2]], t[[0, 2]])  # the valid rows alone, their mean over 2 instead of 4
    assert float(r["loss"][0]) == pytest.approx(float(only["loss"][0]) / 2, rel=1e-12)


# ------------------------------------------------------------------------------------------------ the budgets are not too loose
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("case", cb.POOL_CASES, ids=cb.pool_id)
def test_planted_pool_divisor_is_flagged(case, dtype):
    refs, emu = cb.pool_refs(case, dtype), cb.emulate_pool(cb.pool_inputs(case, dtype), case, dtype, count=case.HW + 1)
    for k in ("fwd", "bwd"):
        with pytest.raises(AssertionError):
            cb.check(emu[k], *refs[k], f"pool {k}", spatial=False)


@pytest.mark.parametrize("case", cb.LIN_CASES, ids=cb.lin_id)
def test_planted_dw_without_the_last_sample_is_flagged(case):
    refs, emu = cb.lin_refs(case), cb.emulate_linear(cb.lin_inputs(case), drop_last=True)
    with pytest.raises(AssertionError):
        cb.check(emu["dw"], *refs["dw"], "dw", spatial=False)
    cb.check(emu["dx"], *refs["dx"], "dx", spatial=False)  # (the other outputs of the same emulation stay inside)


def test_planted_xent_defects_are_flagged():
    c = cb.LIN_CASES[1]  # B = 3
    z, t = cb.xent_logits(c), cb.xent_targets(c)
    refs = cb.xent_refs(z, t)
    assert cb.xent_mismatches(cb.emulate_xent(z, t, no_inv_b=True), refs, "no 1/B") == ["dlogits"]
    # a target at N - 1 (the last row of every case) refused as out of range: the flag, the loss and that row's gradient
    assert cb.xent_mismatches(cb.emulate_xent(z, t, last_class_invalid=True), refs, "N-1 refused") == ["loss", "dlogits", "flags"]
    # hit-5 as rank <= 5: rows 2 and 3 of the tie case have rank exactly 5
    zt, tt, _ = cb.tie_case()
    assert cb.xent_mismatches(cb.emulate_xent(zt, tt, le_for_lt=True), cb.xent_refs(zt, tt), "<= for <") == ["top5"]


def test_softmax_without_max_subtraction_at_logits_of_80_and_of_90():
    """The un-subtracted softmax in plain fp32 (exp, fp32 sum, fp32 log, p = e / sum) on the +-80 case, and on the same logits at +-90.
    At +-80 it is NOT a numerical defect and no budget derived from the formats can call it one: fp32 holds exp(80) = 5.5e34 and the sum
    of a thousand of them (FLT_MAX = 3.4e38; expf overflows from 88.73 on), exp(-80) = 1.8e-35 is a normal number, and skipping the
    subtraction even saves the rounding of z - max.  The emulation of that form stays inside every budget there, and this test says so
    rather than planting a failure that the arithmetic does not have.  At +-90, the first round magnitude past 88.73, exp overflows, the
    probabilities of the rows that hold such a logit are inf / inf, and both the loss and the gradient are flagged.  The subtracted
    emulation is inside the budgets at both scales."""
    c = cb.LIN_CASES[3]
    assert c.scale == 80.0
    z, t = cb.xent_logits(c), cb.xent_targets(c)
    assert float(z.abs().max()) == pytest.approx(80.0, rel=1e-6) and float(z.min()) < -60
    found = {}
    for scale in (80.0, 90.0):
        zs = (z.double() * (scale / 80.0)).float()
        refs = cb.xent_refs(zs, t)
        assert cb.xent_mismatches(cb.emulate_xent(zs, t), refs, f"+-{scale}") == []
        found[scale] = cb.xent_mismatches(cb.emulate_xent(zs, t, no_max=True), refs, f"no max, +-{scale}")
    assert found == {80.0: [], 90.0: ["loss", "dlogits"]}, found


# ------------------------------------------------------------------------------------------------ the head's conv shapes
def test_head_conv_shapes_are_accepted_by_the_planners(pkg):
    lib = pkg._lib.load()
    for c in cb.HEAD_CONV_CASES:
        Wo = c.W // c.stride
        assert lib.hh_conv2d_config(c.cin, c.cout, c.ks, c.stride, 0, Wo) >= 0, tb.conv_id(c)
        assert lib.hh_conv2d_config(c.cin, c.cout, c.ks, c.stride, 2 if c.stride == 2 else 1, Wo) >= 0, tb.conv_id(c)
        plan = (ctypes.c_int * 3)()
        assert lib.hh_conv2d_wgrad_plan(c.B, c.H, c.W, c.cin, c.cout, c.ks, c.stride, plan) == 0, tb.conv_id(c)
    assert sorted(tb.conv_id(c) for c in cb.HEAD_CONV_CASES if cb.head_conv_pixels(c) < cb.SENSITIVE_MIN_PIXELS) == \
        ["1024to2048-k1s1-2x1x1-p00", "256to256-k3s1-2x1x1-p11", "512to1024-k3s2-2x2x2-p11"]


@pytest.mark.parametrize("case", cb.HEAD_CONV_CASES, ids=tb.conv_id)
def test_head_conv_emulation_within_budget(case):
    refs, emu = tb.conv_refs(case), tb.emulate_conv(tb.conv_inputs(case), case)
    worst = {k: tb.check(emu[k], *refs[k], f"{tb.conv_id(case)} {k}") for k in ("fwd", "dgrad", "dgrad_res")}
    ref, hard, sens = refs["wgrad"]
    worst["wgrad hard"] = tb.check(emu["wgrad"], ref, hard, f"{tb.conv_id(case)} wgrad (hard bound)", spatial=False)
    if cb.head_conv_pixels(case) >= cb.SENSITIVE_MIN_PIXELS:
        worst["wgrad sensitive"] = tb.check(emu["wgrad"], ref, sens, f"{tb.conv_id(case)} wgrad (sensitive bound)", spatial=False)
    print("emulation / allowed", tb.conv_id(case), {k: round(v, 3) for k, v in worst.items()})


# ------------------------------------------------------------------------------------------------ the golden training step
LOGIT_BOUND = 0.04  # of max |logit|: the bound of tests/test_gpu_cls_train.py


def test_golden_step_has_no_row_that_a_logit_bound_could_flip():
    """Every logit may move by LOGIT_BOUND x max|logit| in the 16-bit forward.  A row's hit-1 / hit-5 can then change only if the target's
    logit is closer than that to the largest / fifth largest of the others: no row of the fixture is."""
    g = np.load(os.path.join(GOLDEN, "cls_train_step.npz"))
    z, t = g["logits"], g["targets"]
    bound = LOGIT_BOUND * np.abs(z).max()
    hits = [0, 0]
    for b in range(z.shape[0]):
        others = np.sort(np.delete(z[b], t[b]))[::-1]
        assert abs(z[b, t[b]] - others[0]) > bound and abs(z[b, t[b]] - others[4]) > bound, b
        hits[0] += z[b, t[b]] > others[0]
        hits[1] += z[b, t[b]] > others[4]
    assert 1 - hits[0] / len(t) == float(g["top-1_error"]) and 1 - hits[1] / len(t) == float(g["top-5_error"])
    r = cb.xent_refs(torch.from_numpy(z), torch.from_numpy(t))
    assert (r["top1"], r["top5"]) == tuple(hits) and hits[0] >= 1 and hits[1] > hits[0]
    assert float(r["loss"][0]) == pytest.approx(float(g["loss"]), rel=1e-6)


def test_golden_step_conv_biases_in_front_of_batchnorm_have_noise_gradients():
    g = np.load(os.path.join(GOLDEN, "cls_train_step.npz"))
    names = [str(n) for n in g["grad.names"]]
    norm = dict(zip(names, g["grad.norms"]))
    for conv_bias, bn_bias in [(f"classification_head.downsample_blocks.{i}.0.bias", f"classification_head.downsample_blocks.{i}.1.bias") for i in range(3)] + \
            [("classification_head.final_conv.0.bias", "classification_head.final_conv.1.bias")]:
        assert norm[conv_bias] < 1e-3 * norm[bn_bias], (conv_bias, norm[conv_bias], norm[bn_bias])
