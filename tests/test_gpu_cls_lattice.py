"""-m gpu: the classifier's tail kernels (hh_global_avgpool*, hh_linear_*, hh_softmax_xent) against the fp64 references of
tests/cls_budget.py, element by element within that module's budgets, the pool in bf16 and in fp16; and the classification head's conv
shapes (cls_budget.HEAD_CONV_CASES) through tests/train_budget.py's conv_inputs / conv_refs / check as they stand.  Every call is
repeated once for identical bits.

The weight gradient's sensitive bound applies from 48 summed pixels on (cls_budget.SENSITIVE_MIN_PIXELS, with the reference-side figures
behind it); the three two-pixel cases take the hard bound only.
"""
import importlib

import pytest
import torch

import cls_budget as cb
import train_budget as tb
from conftest import PKG

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.bfloat16, torch.float16]


def _ops():
    return importlib.import_module(PKG + ".keypoints.train_ops")


def _same(a, b, what):
    assert a.shape == b.shape and torch.equal(a, b), f"{what}: {int((a != b).sum())} of {a.numel()} values differ"


def _twice(fn, what):
    """fn() -> tensor or tuple of tensors / None; runs it twice and demands identical bits"""
    a, b = fn(), fn()
    for i, (x, y) in enumerate(zip(a, b) if isinstance(a, tuple) else [(a, b)]):
        if x is not None:
            _same(x, y, f"{what}[{i}]: second call vs first")
    return a


# ---------------------------------------------------------------------------------------------------------------- pool
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("case", cb.POOL_CASES, ids=cb.pool_id)
def test_global_avgpool_forward_and_backward(pkg, case, dtype):
    ops, i, refs = _ops(), cb.pool_inputs(case, dtype), cb.pool_refs(case, dtype)
    # [B, HW, C] is the memory of a channels_last [B, C, HW, 1] tensor
    x = i["x"].to(DEV, dtype).permute(0, 2, 1).unsqueeze(-1)
    fwd = _twice(lambda: ops.global_avgpool(x), "pool forward")
    bwd = _twice(lambda: ops.global_avgpool_backward(i["g"].to(DEV), case.HW, 1, dtype), "pool backward")
    assert fwd.dtype == torch.float32 and fwd.shape == (case.B, case.C) and bwd.dtype == dtype and bwd.shape == (case.B, case.C, case.HW, 1)
    r = {"fwd": cb.check(fwd.cpu(), *refs["fwd"], f"pool {cb.pool_id(case)} forward", spatial=False),
         "bwd": cb.check(bwd.float().cpu().squeeze(-1).permute(0, 2, 1), *refs["bwd"], f"pool {cb.pool_id(case)} backward", spatial=False)}
    print(f"engine / allowed pool {cb.pool_id(case)} {dtype}: { {k: round(v, 3) for k, v in r.items()} }")


def test_unsuffixed_pool_entry_points_are_bf16(pkg):
    lib, ops = pkg._lib.load(), _ops()
    case = cb.POOL_CASES[2]
    i = cb.pool_inputs(case, torch.bfloat16)
    x, g = i["x"].to(DEV, torch.bfloat16).contiguous(), i["g"].to(DEV)
    out, dx = torch.empty(case.B, case.C, device=DEV), torch.empty(case.B, case.HW, case.C, device=DEV, dtype=torch.bfloat16)
    stream = torch.cuda.current_stream().cuda_stream
    pkg._lib.check(lib.hh_global_avgpool(x.data_ptr(), case.B, case.HW, case.C, out.data_ptr(), stream))
    pkg._lib.check(lib.hh_global_avgpool_backward(g.data_ptr(), case.B, case.HW, case.C, dx.data_ptr(), stream))
    _same(out, ops.global_avgpool(x.permute(0, 2, 1).unsqueeze(-1)), "hh_global_avgpool vs its _act form with HH_ACT_BF16")
    _same(dx, ops.global_avgpool_backward(g, case.HW, 1, torch.bfloat16).squeeze(-1).permute(0, 2, 1), "hh_global_avgpool_backward vs its _act form")
    assert lib.hh_global_avgpool_act(2, x.data_ptr(), case.B, case.HW, case.C, out.data_ptr(), stream) == 1  # an unknown dtype is refused
    assert lib.hh_global_avgpool(x.data_ptr(), case.B, case.HW, 12, out.data_ptr(), stream) == 1            # C % 8


# ---------------------------------------------------------------------------------------------------------------- linear
@pytest.mark.parametrize("case", cb.LIN_CASES, ids=cb.lin_id)
def test_linear_forward_and_backward(pkg, case):
    ops, refs = _ops(), cb.lin_refs(case)
    i = {k: v.to(DEV) for k, v in cb.lin_inputs(case).items()}
    fwd = _twice(lambda: ops.linear_forward(i["x"], i["w"], i["bias"]), "linear forward")
    dx, dw, db = _twice(lambda: ops.linear_backward(i["x"], i["w"], i["dy"]), "linear backward")
    r = {k: round(cb.check(t.cpu(), *refs[k], f"linear {cb.lin_id(case)} {k}", spatial=False), 3) for k, t in (("fwd", fwd), ("dx", dx), ("dw", dw), ("db", db))}
    print(f"engine / allowed linear {cb.lin_id(case)}: {r}")
    only_dw = ops.linear_backward(i["x"], i["w"], i["dy"], want=(False, True, False))
    assert only_dw[0] is None and only_dw[2] is None
    _same(only_dw[1], dw, "dW computed alone")
    only_dx = ops.linear_backward(i["x"], i["w"], i["dy"], want=(True, False, False))
    assert only_dx[1] is None and only_dx[2] is None
    _same(only_dx[0], dx, "dX computed alone")


# ---------------------------------------------------------------------------------------------------------------- cross-entropy
def _xent(ops, z, t, want_grad=True):
    def call():
        result, dz = ops.softmax_xent(z.to(DEV), t.to(DEV), want_grad=want_grad)
        return result, dz
    result, dz = _twice(call, "softmax_xent")
    r = result.cpu()
    return {"loss": r[:1].view(torch.float32).clone(), "dlogits": dz.cpu() if dz is not None else None, "top1": int(r[1]), "top5": int(r[2]),
            "flags": int(r[3])}, result


@pytest.mark.parametrize("case", cb.LIN_CASES, ids=cb.lin_id)
def test_softmax_xent_vs_fp64(pkg, case):
    ops = _ops()
    z, t = cb.xent_logits(case), cb.xent_targets(case)
    got, result = _xent(ops, z, t)
    refs = cb.xent_refs(z, t)
    r = {k: round(cb.check(got[k], *refs[k], f"xent {cb.lin_id(case)} {k}", spatial=False), 3) for k in ("loss", "dlogits")}
    print(f"engine / allowed xent {cb.lin_id(case)}: {r}; hits {got['top1']} / {got['top5']} of {case.B}")
    assert (got["top1"], got["top5"], got["flags"]) == (refs["top1"], refs["top5"], 0)
    m = ops.read_xent_result(result, case.B)
    assert m["loss"] == float(got["loss"]) and m["top-1_error"] == 1 - refs["top1"] / case.B and m["top-5_error"] == 1 - refs["top5"] / case.B
    nograd, _ = _xent(ops, z, t, want_grad=False)
    assert nograd["dlogits"] is None and torch.equal(nograd["loss"], got["loss"]) and (nograd["top1"], nograd["top5"]) == (got["top1"], got["top5"])


def test_softmax_xent_ties_go_to_the_lower_index(pkg):
    ops = _ops()
    z, t, (top1, top5) = cb.tie_case()
    got, _ = _xent(ops, z, t)
    assert cb.xent_mismatches(got, cb.xent_refs(z, t), "ties") == []
    assert (got["top1"], got["top5"], got["flags"]) == (top1, top5, 0)


def test_softmax_xent_out_of_range_target_sets_the_flag(pkg):
    ops = _ops()
    z, t = cb.out_of_range_case()
    got, result = _xent(ops, z, t)
    assert cb.xent_mismatches(got, cb.xent_refs(z, t), "out of range") == []
    assert got["flags"] == 1 and float(got["dlogits"][1].abs().max()) == 0.0 and float(got["dlogits"][3].abs().max()) == 0.0
    with pytest.raises(IndexError):
        ops.read_xent_result(result, z.shape[0])
    loss_mod = importlib.import_module(PKG + ".classification.loss")
    fn = loss_mod.ClassificationLoss()
    fn.calculate_loss(t.to(DEV), z.to(DEV))  # does not wait for the device, so it cannot raise here ...
    with pytest.raises(IndexError):          # ... reading the record does
        fn.metrics()


def test_classification_loss_takes_part_in_autograd(pkg):
    loss_mod = importlib.import_module(PKG + ".classification.loss")
    case = cb.LIN_CASES[1]
    z, t = cb.xent_logits(case).to(DEV).requires_grad_(), cb.xent_targets(case).to(DEV)
    fn = loss_mod.ClassificationLoss()
    loss = fn.calculate_loss(t, z)
    (loss * 4.0).backward()  # (a power of two: the scaling of the stored gradient is exact)
    refs = cb.xent_refs(z.detach().cpu(), t.cpu())
    cb.check(loss.detach().cpu().reshape(1), *refs["loss"], "loss", spatial=False)
    cb.check(z.grad.cpu() / 4.0, *refs["dlogits"], "dlogits through backward", spatial=False)
    assert fn.metrics()["loss"] == loss.item()


# ---------------------------------------------------------------------------------------------------------------- the head's convs
@pytest.mark.parametrize("case", cb.HEAD_CONV_CASES, ids=tb.conv_id)
def test_head_conv_shapes_vs_fp64_within_budget(pkg, case):
    ops, i, refs = _ops(), tb.conv_inputs(case), tb.conv_refs(case)

    def d(t):
        return t.to(DEV, torch.bfloat16).contiguous(memory_format=torch.channels_last)

    def calls():
        x, dy, w = d(i["x"]), d(i["dy"]), i["w"].to(DEV)
        return {"fwd": ops.conv2d(x, w, case.stride, bias=i["bias"].to(DEV), res=d(i["res"]), relu=True),
                "dgrad": ops.conv2d(dy, w, case.stride, data_grad=True),
                "dgrad_res": ops.conv2d(dy, w, case.stride, data_grad=True, res=d(i["gres"])),
                "wgrad": ops.conv2d_weight_grad(x, dy, case.ks, case.stride)}
    got, again = calls(), calls()
    for k in got:
        _same(again[k], got[k], f"{tb.conv_id(case)} {k}: second call vs first")
    ratios = {k: round(tb.check(got[k].float().cpu(), *refs[k], f"{tb.conv_id(case)} {k}"), 3) for k in ("fwd", "dgrad", "dgrad_res")}
    ref, hard, sens = refs["wgrad"]
    ratios["wgrad hard"] = round(tb.check(got["wgrad"].cpu(), ref, hard, f"{tb.conv_id(case)} wgrad, hard bound", spatial=False), 3)
    if cb.head_conv_pixels(case) >= cb.SENSITIVE_MIN_PIXELS:
        ratios["wgrad sensitive"] = round(tb.check(got["wgrad"].cpu(), ref, sens, f"{tb.conv_id(case)} wgrad, sensitive bound", spatial=False), 3)
    print(f"engine / allowed {tb.conv_id(case)}: {ratios}")
