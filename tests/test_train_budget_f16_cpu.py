"""The fp16 budgets of tests/train_budget_f16.py hold what they should, without a GPU: the CPU emulation of the kernels' arithmetic
(torch fp32 on fp16-rounded operands, fp16 where the kernel stores fp16) stays inside every budget on every lattice case, and three
planted defects are flagged: the result stored through bf16 (what launching the bf16 instantiation on an fp16 call would round to;
this pins that the budgets tell the two paths apart, on every case), a saturating store on an overflow case, and subnormal outputs
flushed to zero on a small-magnitude case.

Worst emulation / allowed over the full lattices: conv forward 0.987, data gradient 0.983, with skip 0.990, weight gradient hard 0.104,
sensitive 0.634 (K = 1.0); BatchNorm y 0.999, dx 0.999 (both at C96-2x304x304-res-relu; 0.997 / 0.996 without the two cases above 3 M
elements); fusion sum forward / backward 0.999 (the store's own half ulp fills the budget, as for bf16); subnormal case 0.899 .. 0.928.
Wall time: 26 s for the 67 tests on 8 threads."""
import pytest
import torch

import train_budget_f16 as tbf
from test_train_budget_cpu import _flags


def _as_bf16(fn):
    """fn() with the copy's store rounding through bf16 instead of fp16 (operands built before the call keep their fp16 values)"""
    keep = tbf.bf
    tbf._tb.bf = lambda t: t.to(torch.bfloat16).float()
    try:
        return fn()
    finally:
        tbf._tb.bf = keep


# ------------------------------------------------------------------------------------------------ the budgets are not too tight
@pytest.mark.parametrize("case", tbf.CONV_CASES, ids=tbf.conv_id)
def test_conv_emulation_within_fp16_budget_and_bf16_store_is_flagged(case):
    cid = tbf.conv_id(case)
    i, refs = tbf.conv_inputs(case), tbf.conv_refs(case)
    emu = tbf.emulate_conv(i, case)
    worst = {k: tbf.check(emu[k], *refs[k], f"{cid} {k}") for k in ("fwd", "dgrad", "dgrad_res")}
    ref, hard, sens = refs["wgrad"]
    worst["wgrad hard"] = tbf.check(emu["wgrad"], ref, hard, f"{cid} wgrad (hard bound)", spatial=False)
    worst["wgrad sensitive"] = tbf.check(emu["wgrad"], ref, sens, f"{cid} wgrad (sensitive bound)", spatial=False)
    print("emulation / allowed", cid, {k: round(v, 3) for k, v in worst.items()})
    wrong = _as_bf16(lambda: tbf.emulate_conv(i, case))
    for k in ("fwd", "dgrad", "dgrad_res"):
        _flags(lambda: tbf.check(wrong[k], *refs[k], f"{cid} {k} stored through bf16"))


@pytest.mark.parametrize("case", tbf.BN_CASES, ids=tbf.bn_id)
def test_bn_emulation_within_fp16_budget_and_bf16_store_is_flagged(case):
    cid = tbf.bn_id(case)
    i = tbf.bn_inputs(case)
    fr = tbf.bn_forward_refs(case)
    fw = tbf.emulate_bn_forward(i, case)
    worst = {k: tbf.check(fw[k], *v, f"{cid} {k}", spatial=k == "y") for k, v in fr.items()}
    bw = tbf.emulate_bn_backward(i, case, fw)
    br = tbf.bn_backward_refs(case, fw["y"])
    for k, v in br.items():
        worst[k] = tbf.check(bw[k], *v, f"{cid} {k}", spatial=k in ("dx", "dres"))
    print("emulation / allowed", cid, {k: round(v, 3) for k, v in worst.items()})
    wrong = _as_bf16(lambda: tbf.emulate_bn_forward(i, case))
    _flags(lambda: tbf.check(wrong["y"], *fr["y"], f"{cid} y stored through bf16"))
    if case.B * case.H * case.W > 2:  # (two pixels: xhat = +-1 and dx = g - mean g - xhat mean(g xhat) is 0 up to rounding, whatever the store)
        wrong = _as_bf16(lambda: tbf.emulate_bn_backward(i, case, fw))
        _flags(lambda: tbf.check(wrong["dx"], *br["dx"], f"{cid} dx stored through bf16"))


@pytest.mark.parametrize("case", tbf.FUSION_CASES, ids=tbf.fusion_id)
def test_fusion_emulation_within_fp16_budget_and_bf16_store_is_flagged(case):
    cid = tbf.fusion_id(case)
    i = tbf.fusion_inputs(case)
    out = tbf.emulate_fusion(i, case)
    worst = [tbf.check(out, *tbf.fusion_forward_ref(case), f"{cid} out")]
    refs = tbf.fusion_backward_refs(case, out)
    for j, (g, r) in enumerate(zip(tbf.emulate_fusion_backward(i, case, out), refs)):
        worst.append(tbf.check(g, *r, f"{cid} gradient of term {j}"))
    print("emulation / allowed", cid, [round(v, 3) for v in worst])
    wrong = _as_bf16(lambda: tbf.emulate_fusion(i, case))
    _flags(lambda: tbf.check(wrong, *tbf.fusion_forward_ref(case), f"{cid} out stored through bf16"))
    wrong = _as_bf16(lambda: tbf.emulate_fusion_backward(i, case, out))
    for j, s in enumerate(case.shifts):
        if s > 0:  # (a same-resolution term's gradient is a masked copy: nothing is rounded)
            _flags(lambda: tbf.check(wrong[j], *refs[j], f"{cid} gradient of term {j} stored through bf16"))


def test_the_second_copy_leaves_the_bf16_budgets_alone():
    import train_budget as tb
    assert (tb.U16, tb.K_SENSITIVE) == (2.0 ** -8, 0.5) and (tbf.U16, tbf.K_SENSITIVE, tbf.ETA) == (2.0 ** -11, 1.0, 2.0 ** -25)
    x = torch.tensor([1.0 + 2.0 ** -9, 70000.0, 2.0 ** -20 + 2.0 ** -24])
    assert tb.bf(x).tolist() == [1.0, 70144.0, 2.0 ** -20 + 2.0 ** -24] and tbf.bf(x).tolist() == [1.0 + 2.0 ** -9, float("inf"), 2.0 ** -20 + 2.0 ** -24]
    assert [tuple(c) for c in tbf.CONV_CASES] == [tuple(c) for c in tb.CONV_CASES] and tbf.check.__code__.co_code == tb.check.__code__.co_code


# ------------------------------------------------------------------------------------------------ overflow and subnormals
def test_saturating_store_is_flagged_on_an_overflow_case():
    i = tbf.special_conv_inputs("overflow")
    ref, allowed = tbf.special_conv_refs(i)["fwd"]
    over = int((ref >= tbf.F16_OVER + allowed).sum())
    assert over > 0.2 * ref.numel() and int(((ref > 0) & (ref < tbf.F16_MAX / 2)).sum()) > 0, over  # values on both sides of the limit
    good = tbf.bf(tbf.conv_forward(i, tbf.SPECIAL_CONV))  # fp16 rounding: inf beyond 65520
    assert int(torch.isinf(good).sum()) >= over
    tbf.check_f16(good, ref, allowed, "overflow case, fp16 store")
    saturated = good.clamp(max=tbf.F16_MAX)
    _flags(lambda: tbf.check_f16(saturated, ref, allowed, "overflow case, saturating store"), "inf x allowed", border=">0")
    # an inf where the value is far below the limit is as wrong
    early = good.clone()
    early[0, 0, 2, 3] = float("inf")
    if ref[0, 0, 2, 3] + allowed[0, 0, 2, 3] < tbf.F16_OVER:
        _flags(lambda: tbf.check_f16(early, ref, allowed, "overflow case, inf too early"), "worst at [0, 0, 2, 3]")
    # and so is the inf of the other sign
    wrong_sign = torch.where(torch.isinf(good), -good, good)
    _flags(lambda: tbf.check_f16(wrong_sign, ref, allowed, "overflow case, -inf"), border=">0")


def test_flushed_subnormals_are_flagged_on_a_small_magnitude_case():
    c = tbf.SPECIAL_CONV
    i = tbf.special_conv_inputs("subnormal")
    refs = tbf.special_conv_refs(i)
    assert float(i["w"].abs().max()) < tbf.F16_MIN_NORMAL  # every weight is an fp16 subnormal
    emu = tbf.emulate_conv(i, c)
    for k in ("fwd", "dgrad", "dgrad_res"):
        ref = refs[k][0]
        sub = (ref.abs() >= tbf.F16_MIN_SUBNORMAL) & (ref.abs() < tbf.F16_MIN_NORMAL)
        assert int(sub.sum()) > 0.3 * ref.numel(), (k, int(sub.sum()))
        print("emulation / allowed, subnormal case", k, round(tbf.check(emu[k], *refs[k], f"subnormal case {k}"), 3))
        flushed = torch.where(emu[k].abs() < tbf.F16_MIN_NORMAL, torch.zeros_like(emu[k]), emu[k])
        _flags(lambda: tbf.check(flushed, *refs[k], f"subnormal case {k}, outputs flushed"), border=">0")
    ref, hard, sens = refs["wgrad"]
    tbf.check(emu["wgrad"], ref, sens, "subnormal case wgrad", spatial=False)
    # flushed MFMA inputs (the weights read as zero) leave bias + res alone in the forward and nothing in the data gradient
    j = dict(i, w=torch.zeros_like(i["w"]))
    _flags(lambda: tbf.check(tbf.emulate_conv(j, c)["fwd"], *refs["fwd"], "subnormal case fwd, weights flushed"), border=">0")
    _flags(lambda: tbf.check(tbf.emulate_conv(j, c)["dgrad"], *refs["dgrad"], "subnormal case dgrad, weights flushed"), border=">0")
