"""-m gpu: the training ops on fp16 activations against fp64 references over the lattices of tests/train_budget.py, element by element
within the fp16 budgets of tests/train_budget_f16.py (that module's docstring: u_h = 2^-11, ETA = 2^-25, K = 1.0).

hh_conv2d_dt in its three modes (forward with bias + residual + ReLU, data gradient of a stride-1 / stride-2 conv with and without the
skip gradient), hh_conv2d_wgrad_dt (hard and sensitive bound), the packed-weights path (bit-identical), train_net.conv / deconv_k4s2
with their channel padding, the hh_bn_train_*_dt family (fused, without y, and split around the exchange at world 1: bit-equal to the
fused passes) and hh_fusion_sum_*_dt.  Every call is repeated once for identical bits.

Special values on one small case (32to32-k3s1-1x6x16): a forward whose true value exceeds 65504 gives +inf (no saturation); an inf
and a NaN planted in dy come out as non-finite entries of the data gradient and of dw, and nowhere else; BatchNorm backward with an inf
in dy gives non-finite dgamma / dbeta; operands scaled so that the weights and most outputs are fp16 subnormals stay within budget.
Contract: mixed fp16 / bf16 activations in one call raise HHError, an unknown dtype is refused through hh_last_error, and every _dt
entry point called with bf16 gives the bits of the entry point without the suffix.

Worst engine / allowed ratio per op family on the MI355X (test_report_worst_ratios prints them; 1.0 = at the budget):
  conv forward 0.987   conv data gradient 0.990   BatchNorm forward 0.999   BatchNorm backward 0.999   fusion sum forward / backward 0.999
  conv weight gradient: hard bound 0.073, sensitive bound 0.386   subnormal case 0.928
  train_net.conv / deconv_k4s2: output 0.971, data gradient 0.987, bias gradient 0.704, weight gradient hard 0.010, sensitive 0.119
Wall time of this file on an MI355X, fp64 references included: 7 s for its 115 tests.
"""
import ctypes
import importlib
import time

import pytest
import torch
import torch.nn.functional as F

import train_budget_f16 as tbf
from conftest import PKG

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WORST = {}   # op family -> worst engine / allowed ratio of this process
T0 = time.time()


def _ops():
    return importlib.import_module(PKG + ".keypoints.train_ops")


def _d(t, dtype=torch.float16):
    """fp16 NHWC on the device (the values are fp16-representable already)"""
    return t.to(DEV, dtype).contiguous(memory_format=torch.channels_last)


def _note(family, ratio):
    WORST[family] = max(WORST.get(family, 0.0), ratio)
    return round(ratio, 3)


def _same(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b), f"{what}: {int((a != b).sum())} of {a.numel()} values differ"


# ---------------------------------------------------------------------------------------------------------------- convolutions
def _conv_calls(ops, c, i, packed=None, dtype=torch.float16):
    """the four calls of one case -> {fwd, dgrad, dgrad_res, wgrad}; packed: (forward, data-gradient) buffers of PackedConvWeights"""
    pad = c.pad if c.ks == 2 else None  # (3x3 and 1x1 take the default, as train_net does)
    x, dy, w = _d(i["x"], dtype), _d(i["dy"], dtype), i["w"].to(DEV)
    pf, pb = packed or (None, None)
    bias = i["bias"].to(DEV) if (packed is None or c.cout % 32 == 0) else None  # the packed call takes a bias of a multiple of 32 entries only
    out = {"fwd": ops.conv2d(x, w, c.stride, bias=bias, res=_d(i["res"], dtype), relu=True, pad=pad, packed=pf),
           "dgrad": ops.conv2d(dy, w, c.stride, data_grad=True, pad=pad, packed=pb),
           "dgrad_res": ops.conv2d(dy, w, c.stride, data_grad=True, pad=pad, packed=pb, res=_d(i["gres"], dtype))}
    if packed is None:
        out["wgrad"] = ops.conv2d_weight_grad(x, dy, c.ks, c.stride, pad=pad)
    elif bias is None:
        out["fwd_ref"] = ops.conv2d(x, w, c.stride, res=_d(i["res"], dtype), relu=True, pad=pad)  # what the packed forward must equal
    for k, v in out.items():
        assert v.dtype == (torch.float32 if k == "wgrad" else dtype), (k, v.dtype)
    return out


@pytest.mark.parametrize("case", tbf.CONV_CASES, ids=tbf.conv_id)
def test_conv_ops_fp16_vs_fp64_within_budget(pkg, case):
    ops, i, refs = _ops(), tbf.conv_inputs(case), tbf.conv_refs(case)
    got = _conv_calls(ops, case, i)
    again = _conv_calls(ops, case, i)
    for k in got:
        _same(again[k], got[k], f"{tbf.conv_id(case)} {k}: second call vs first")
    ratios = {}
    for k, fam in (("fwd", "conv forward"), ("dgrad", "conv data gradient"), ("dgrad_res", "conv data gradient")):
        ratios[k] = _note(fam, tbf.check(got[k].float().cpu(), *refs[k], f"{tbf.conv_id(case)} {k}"))
    ref, hard, sens = refs["wgrad"]
    ratios["wgrad hard"] = _note("conv weight gradient (hard)", tbf.check(got["wgrad"].cpu(), ref, hard, f"{tbf.conv_id(case)} wgrad, hard bound", spatial=False))
    ratios["wgrad sensitive"] = _note("conv weight gradient (sensitive)",
                                      tbf.check(got["wgrad"].cpu(), ref, sens, f"{tbf.conv_id(case)} wgrad, sensitive bound", spatial=False))
    print(f"engine / allowed {tbf.conv_id(case)}: {ratios}")


@pytest.mark.parametrize("case", tbf.CONV_CASES, ids=tbf.conv_id)
def test_conv_packed_fp16_weights_same_bits(pkg, case):
    ops, i = _ops(), tbf.conv_inputs(case)
    w = i["w"].to(DEV)
    pw = ops.PackedConvWeights([(w, case.stride, False), (w, case.stride, True)], dtype=torch.float16)
    assert all(b.dtype == torch.float16 for b in pw.buffers)
    pw.refresh()
    plain, packed = _conv_calls(ops, case, i), _conv_calls(ops, case, i, packed=tuple(pw.buffers))
    _same(packed["fwd"], packed.get("fwd_ref", plain["fwd"]), f"{tbf.conv_id(case)} packed forward")
    _same(packed["dgrad"], plain["dgrad"], f"{tbf.conv_id(case)} packed data gradient")
    _same(packed["dgrad_res"], plain["dgrad_res"], f"{tbf.conv_id(case)} packed data gradient with res")


# ---------------------------------------------------------------------------------------------------------------- wrappers
def _wgrad_checks(got, ref, n, S, what):
    r = _note("wrapper weight gradient (hard)", tbf.check(got, ref, (n + 2) * tbf.U32 * S, what + ", hard bound", spatial=False))
    s = _note("wrapper weight gradient (sensitive)", tbf.check(got, ref, tbf.K_SENSITIVE * n ** 0.5 * tbf.U32 * S, what + ", sensitive bound", spatial=False))
    return r, s


@pytest.mark.parametrize("cin,cout,ks,stride,shape", [(3, 64, 3, 2, (3, 12, 40)), (32, 17, 1, 1, (3, 6, 17)), (32, 34, 1, 1, (5, 3, 24)), (66, 32, 3, 1, (3, 6, 40))],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_train_net_conv_channel_padding_fp16(pkg, cin, cout, ks, stride, shape):
    """train_net.conv pads 3 -> 16, 17 -> 32, 34 -> 48, 66 -> 80 channels and slices the result back; the bias is an fp16 add behind the
    kernel.  Budgets: the conv's own, then one more fp16 rounding (u_h and ETA) for the bias add; the gradients' are the ops' (padding and
    slicing copy); the bias gradient is an fp16-rounded fp32 sum."""
    tn = importlib.import_module(PKG + ".keypoints.train_net")
    B, H, W = shape
    g = torch.Generator().manual_seed(4000 + cin)
    m = torch.nn.Conv2d(cin, cout, ks, stride, (ks - 1) // 2, bias=True)
    with torch.no_grad():
        m.weight.copy_(tbf.bf(torch.randn(m.weight.shape, generator=g) * (2.0 / (cin * ks * ks)) ** 0.5))
        m.bias.copy_(tbf.bf(torch.randn(cout, generator=g)))
    x = tbf.bf(torch.randn(B, cin, H, W, generator=g))
    dy = tbf.bf(torch.randn(B, cout, H // stride, W // stride, generator=g))
    xr, wr, br = x.double().requires_grad_(), m.weight.detach().double().requires_grad_(), m.bias.detach().double().requires_grad_()
    r1 = F.conv2d(xr, wr, None, stride, (ks - 1) // 2)
    (r1 + br.view(1, -1, 1, 1)).backward(dy.double())
    xa, wa = x.double().abs().requires_grad_(), m.weight.detach().double().abs().requires_grad_()
    s1 = F.conv2d(xa, wa, None, stride, (ks - 1) // 2)
    s1.backward(dy.double().abs())
    m = m.to(DEV)
    xd = _d(x).requires_grad_()
    y = tn.conv(xd, m)
    assert y.dtype == torch.float16
    y.backward(_d(dy))
    a1 = tbf._stored(r1.detach(), cin * ks * ks, s1.detach())
    ref = (r1 + br.view(1, -1, 1, 1)).detach()
    what = f"train_net.conv fp16 {cin}->{cout} k{ks}s{stride}"
    ratios = {"y": _note("wrapper output", tbf.check(y.detach().float().cpu(), ref, a1 + tbf.U16 * (ref.abs() + a1) + tbf.ETA, what + " output")),
              "dx": _note("wrapper data gradient", tbf.check(xd.grad.float().cpu(), xr.grad, tbf._stored(xr.grad, cout * ks * ks, xa.grad), what + " dx"))}
    n = dy.shape[0] * dy.shape[2] * dy.shape[3]
    ratios["dw"] = _wgrad_checks(m.weight.grad.cpu(), wr.grad, n, wa.grad, what + " dw")
    sb = dy.double().abs().sum((0, 2, 3))
    ratios["dbias"] = _note("wrapper bias gradient", tbf.check(m.bias.grad.cpu(), br.grad, tbf._stored(br.grad, n, sb), what + " dbias", spatial=False))
    print(f"engine / allowed {what}: {ratios}")


@pytest.mark.parametrize("cin,cout,shape", [(66, 32, (3, 3, 17)), (82, 48, (1, 6, 24))], ids=str)
def test_train_net_deconv_k4s2_fp16(pkg, cin, cout, shape):
    """ConvTranspose2d(k 4, s 2, p 1) as four 2x2 phase convs with asymmetric padding.  Output: each element is one phase conv's (n = 4 cin);
    dx: the four phases' data gradients, each rounded to fp16, added by autograd in fp16 (three more roundings: u_h and ETA each); dw: every
    tap belongs to one phase, so the weight gradient is that phase's."""
    tn = importlib.import_module(PKG + ".keypoints.train_net")
    B, H, W = shape
    g = torch.Generator().manual_seed(5000 + cin)
    m = torch.nn.ConvTranspose2d(cin, cout, 4, 2, 1, bias=False)
    with torch.no_grad():
        m.weight.copy_(tbf.bf(torch.randn(m.weight.shape, generator=g) * (2.0 / (cin * 4)) ** 0.5))
    x, dy = tbf.bf(torch.randn(B, cin, H, W, generator=g)), tbf.bf(torch.randn(B, cout, 2 * H, 2 * W, generator=g))

    def grads(xv, wv, dyv):
        xv, wv = xv.clone().requires_grad_(), wv.clone().requires_grad_()
        out = F.conv_transpose2d(xv, wv, None, 2, 1)
        out.backward(dyv)
        return out.detach(), xv.grad, wv.grad

    w64 = m.weight.detach().double()
    ref, dx, dw = grads(x.double(), w64, dy.double())
    S, sx, sw = grads(x.double().abs(), w64.abs(), dy.double().abs())
    a_dx, partial = 0, 0
    for py in range(2):
        for px in range(2):
            mask = torch.zeros_like(dy, dtype=torch.float64)
            mask[:, :, py::2, px::2] = 1
            r_p = grads(x.double(), w64, dy.double() * mask)[1]
            s_p = grads(x.double().abs(), w64.abs(), dy.double().abs() * mask)[1]
            a_p = tbf._stored(r_p, cout * 4, s_p)
            a_dx, partial = a_dx + a_p, partial + r_p.abs() + a_p
    a_dx = a_dx + 3 * (tbf.U16 * partial + tbf.ETA)
    m = m.to(DEV)
    xd = _d(x).requires_grad_()
    y = tn.deconv_k4s2(xd, m)
    assert y.dtype == torch.float16
    y.backward(_d(dy))
    what = f"deconv_k4s2 fp16 {cin}->{cout} {shape}"
    ratios = {"y": _note("wrapper output", tbf.check(y.detach().float().cpu(), ref, tbf._stored(ref, cin * 4, S), what + " output")),
              "dx": _note("wrapper data gradient", tbf.check(xd.grad.float().cpu(), dx, a_dx, what + " dx")),
              "dw": _wgrad_checks(m.weight.grad.cpu(), dw, B * H * W, sw, what + " dw")}
    print(f"engine / allowed {what}: {ratios}")


# ---------------------------------------------------------------------------------------------------------------- BatchNorm
@pytest.mark.parametrize("case", tbf.BN_CASES, ids=tbf.bn_id)
def test_batchnorm_ops_fp16_vs_fp64_within_budget(pkg, case, monkeypatch):
    ops, i, cid = _ops(), tbf.bn_inputs(case), tbf.bn_id(case)
    x, dy, res = _d(i["x"]), _d(i["dy"]), _d(i["res"]) if case.res else None
    gamma, beta = i["gamma"].to(DEV), i["beta"].to(DEV)
    fr = tbf.bn_forward_refs(case)
    ratios = {}
    y, mean, invstd = ops.bn_train_forward(x, gamma, beta, tbf.BN_EPS, res, case.relu)
    assert y.dtype == torch.float16 and mean.dtype == invstd.dtype == torch.float32
    y2, mean2, invstd2 = ops.bn_train_forward(x, gamma, beta, tbf.BN_EPS, res, case.relu)
    _same(y2, y, f"{cid} y: second call vs first"); _same(mean2, mean, f"{cid} mean again"); _same(invstd2, invstd, f"{cid} invstd again")
    for k, v, sp in (("mean", mean, False), ("invstd", invstd, False), ("y", y.float(), True)):
        ratios[k] = _note("BatchNorm forward", tbf.check(v.cpu(), *fr[k], f"{cid} {k}", spatial=sp))
    br = tbf.bn_backward_refs(case, y.float())
    out = ops.bn_train_backward(x, y, dy, mean, invstd, gamma, case.relu, want_dres=case.res)
    for k, v in zip(("dx", "dgamma", "dbeta", "dres"), out):
        if k in br:
            assert v.dtype == (torch.float16 if k in ("dx", "dres") else torch.float32)
            ratios[k] = _note("BatchNorm backward", tbf.check(v.float().cpu(), *br[k], f"{cid} {k}", spatial=k in ("dx", "dres")))
        else:
            assert v is None
    for a, b in zip(ops.bn_train_backward(x, y, dy, mean, invstd, gamma, case.relu, want_dres=case.res), out):
        assert (a is None and b is None) or torch.equal(a, b), f"{cid} backward: second call vs first"
    if not case.res:  # without a residual the backward can do without y: the same bits
        plain = ops.bn_train_backward(x, None, dy, mean, invstd, gamma, case.relu, beta=beta)
        for k, a, b in zip(("dx", "dgamma", "dbeta"), plain, out):
            _same(a, b, f"{cid} backward without y, {k}")
    # the split entry points at world 1 (no exchange): the fused passes, bit for bit
    monkeypatch.setattr(ops, "_all_reduce_sums", lambda sums, group: None)
    ys, ms, iss, count = ops.sync_bn_train_forward(x, gamma, beta, tbf.BN_EPS, res, case.relu, None, 1)
    assert count == case.B * case.H * case.W
    _same(ys, y, f"{cid} split forward y"); _same(ms, mean, f"{cid} split forward mean"); _same(iss, invstd, f"{cid} split forward invstd")
    for k, a, b in zip(("dx", "dgamma", "dbeta", "dres"), ops.sync_bn_train_backward(x, ys, dy, ms, iss, gamma, case.relu, case.res, None, count), out):
        assert (a is None and b is None) or (a.dtype == b.dtype and torch.equal(a, b)), f"{cid} split backward {k}"
    print(f"engine / allowed {cid}: {ratios}")


# ---------------------------------------------------------------------------------------------------------------- fusion sum
@pytest.mark.parametrize("case", tbf.FUSION_CASES, ids=tbf.fusion_id)
def test_fusion_sum_fp16_vs_fp64_within_budget(pkg, case):
    ops, i, cid = _ops(), tbf.fusion_inputs(case), tbf.fusion_id(case)
    terms, dy, shifts = [_d(t) for t in i["terms"]], _d(i["dy"]), list(case.shifts)
    out = ops.fusion_sum(terms, shifts, relu=case.relu)
    assert out.dtype == torch.float16
    _same(ops.fusion_sum(terms, shifts, relu=case.relu), out, f"{cid} out: second call vs first")
    ratios = [_note("fusion sum forward", tbf.check(out.float().cpu(), *tbf.fusion_forward_ref(case), f"{cid} out"))]
    grads = ops.fusion_sum_backward(dy, out, shifts, relu=case.relu)
    again = ops.fusion_sum_backward(dy, out, shifts, relu=case.relu)
    assert len(grads) == len(shifts)
    for j, (gj, rj) in enumerate(zip(grads, tbf.fusion_backward_refs(case, out.float()))):
        _same(again[j], gj, f"{cid} gradient of term {j}: second call vs first")
        ratios.append(_note("fusion sum backward", tbf.check(gj.float().cpu(), *rj, f"{cid} gradient of term {j} (shift {shifts[j]})")))
        if not case.relu and shifts[j] == 0:
            assert gj.data_ptr() == dy.data_ptr(), f"{cid}: without ReLU the gradient of a same-resolution term is dy itself"
    print(f"engine / allowed {cid}: {ratios}")


# ---------------------------------------------------------------------------------------------------------------- special values
def _special_calls(ops, i):
    return _conv_calls(ops, tbf.SPECIAL_CONV, i)


def test_overflow_gives_inf_not_the_largest_finite_value(pkg):
    ops = _ops()
    i = tbf.special_conv_inputs("overflow")
    ref, allowed = tbf.special_conv_refs(i)["fwd"]
    got = _special_calls(ops, i)["fwd"].float().cpu()
    must = ref - allowed >= tbf.F16_OVER
    assert int(must.sum()) > 0.2 * ref.numel()
    assert not got.isnan().any() and bool((got[must] == float("inf")).all()), "a value beyond 65504 must be stored as +inf"
    print("overflow case engine / allowed (finite part):", _note("conv forward", tbf.check_f16(got, ref, allowed, "overflow case fwd")))


def test_inf_and_nan_in_dy_reach_the_data_gradient_and_dw(pkg):
    ops, c = _ops(), tbf.SPECIAL_CONV
    i = dict(tbf.conv_inputs(c))
    dy = i["dy"].clone()
    dy[0, 3, 2, 5], dy[0, 7, 4, 9] = float("inf"), float("nan")
    i["dy"] = dy
    got = _special_calls(ops, i)
    hit = torch.zeros(c.H, c.W, dtype=torch.bool)
    hit[1:4, 4:7] = hit[3:6, 8:11] = True  # the 3 x 3 neighbourhoods of the two planted pixels
    for k in ("dgrad", "dgrad_res"):
        bad = ~torch.isfinite(got[k].float().cpu())[0]
        assert bool(bad[:, hit].all()) and not bool(bad[:, ~hit].any()), f"{k}: non-finite at {int(bad.sum())} elements, expected every channel of 18 pixels"
    bad = ~torch.isfinite(got["wgrad"].cpu())
    assert bool(bad[3].all()) and bool(bad[7].all()) and int(bad.sum()) == 2 * c.cin * 9, f"dw: {int(bad.sum())} non-finite entries, expected rows 3 and 7"
    assert bool(got["wgrad"][7].isnan().all())


def test_batchnorm_backward_inf_in_dy_reaches_dgamma_and_dbeta(pkg):
    ops = _ops()
    case = next(c for c in tbf.BN_CASES if tbf.bn_id(c) == "C16-1x1x97")  # no ReLU: no mask stands between dy and the sums
    i = tbf.bn_inputs(case)
    x, gamma, beta = _d(i["x"]), i["gamma"].to(DEV), i["beta"].to(DEV)
    dy = i["dy"].clone()
    dy[0, 5, 0, 40] = float("inf")
    y, mean, invstd = ops.bn_train_forward(x, gamma, beta, tbf.BN_EPS, None, False)
    for out in (ops.bn_train_backward(x, y, _d(dy), mean, invstd, gamma, False), ops.bn_train_backward(x, None, _d(dy), mean, invstd, gamma, False, beta=beta)):
        dx, dgamma, dbeta = (t.float().cpu() for t in out[:3])
        for name, v in (("dgamma", dgamma), ("dbeta", dbeta)):
            bad = ~torch.isfinite(v)
            assert bool(bad[5]) and int(bad.sum()) == 1, f"{name}: non-finite at {bad.nonzero().flatten().tolist()}, expected channel 5 alone"
        bad = ~torch.isfinite(dx)
        assert bool(bad[:, 5].all()) and int(bad.sum()) == 97, "dx: channel 5 takes dbeta / P at every pixel"


def test_subnormal_operands_and_outputs_within_budget(pkg):
    """The weights (about 2^-20) are fp16 subnormals, and so are most outputs and data gradients: MFMA inputs, the epilogue's residual
    unpack and the stores all have to keep them.  Budget: the lattice's, u_h (|ref| + A) + A + ETA, nothing added."""
    ops = _ops()
    i = tbf.special_conv_inputs("subnormal")
    refs = tbf.special_conv_refs(i)
    assert float(i["w"].abs().max()) < tbf.F16_MIN_NORMAL
    got = _special_calls(ops, i)
    ratios = {}
    for k in ("fwd", "dgrad", "dgrad_res"):
        ref = refs[k][0]
        assert int(((ref.abs() >= tbf.F16_MIN_SUBNORMAL) & (ref.abs() < tbf.F16_MIN_NORMAL)).sum()) > 0.3 * ref.numel()
        g = got[k].float().cpu()
        print(f"subnormal case {k}: {int((g != 0).sum())} of {g.numel()} stored values non-zero, {int(((g != 0) & (g.abs() < tbf.F16_MIN_NORMAL)).sum())} subnormal")
        ratios[k] = _note("subnormal case", tbf.check(g, *refs[k], f"subnormal case {k}"))
    ref, hard, sens = refs["wgrad"]
    ratios["wgrad sensitive"] = _note("subnormal case", tbf.check(got["wgrad"].cpu(), ref, sens, "subnormal case wgrad", spatial=False))
    print(f"engine / allowed, subnormal case: {ratios}")


# ---------------------------------------------------------------------------------------------------------------- contract
def test_mixed_activation_types_raise(pkg):
    ops, c = _ops(), tbf.SPECIAL_CONV
    i = tbf.conv_inputs(c)
    x, dy, w = _d(i["x"]), _d(i["dy"]), i["w"].to(DEV)
    xb, dyb = _d(i["x"], torch.bfloat16), _d(i["dy"], torch.bfloat16)
    gamma, beta = torch.ones(c.cin, device=DEV), torch.zeros(c.cin, device=DEV)
    pw = ops.PackedConvWeights([(w, 1, False)])  # bf16 buffers
    y, mean, invstd = ops.bn_train_forward(x, gamma, beta)
    calls = {
        "conv2d res": lambda: ops.conv2d(x, w, res=dyb),
        "conv2d packed": lambda: ops.conv2d(x, w, packed=pw.buffers[0]),
        "conv2d_weight_grad": lambda: ops.conv2d_weight_grad(x, dyb, 3),
        "bn_train_forward res": lambda: ops.bn_train_forward(x, gamma, beta, res=xb),
        "bn_train_backward": lambda: ops.bn_train_backward(x, y, dyb, mean, invstd, gamma),
        "bn_train_backward plain": lambda: ops.bn_train_backward(x, None, dyb, mean, invstd, gamma, beta=beta),
        "sync_bn_train_forward res": lambda: ops.sync_bn_train_forward(x, gamma, beta, 1e-5, xb, False, None, 1),
        "sync_bn_train_backward": lambda: ops.sync_bn_train_backward(x, y, dyb, mean, invstd, gamma, False, False, None, float(c.H * c.W)),
        "fusion_sum": lambda: ops.fusion_sum([x, xb], [0, 0]),
        "fusion_sum_backward": lambda: ops.fusion_sum_backward(dy, xb, [0, 0]),
    }
    for name, fn in calls.items():
        with pytest.raises(pkg._lib.HHError, match="one element type"):
            fn()
        print("refused:", name)
    with pytest.raises(pkg._lib.HHError):
        ops.conv2d(x.float(), w)
    with pytest.raises(pkg._lib.HHError):
        ops.PackedConvWeights([(w, 1, False)], dtype=torch.float32)
    # an unknown dtype at the C-ABI: an error through hh_last_error, nothing launched
    lib = pkg._lib.load()
    out = torch.empty_like(x)
    ptrs, sh = (ctypes.c_void_p * 1)(x.data_ptr()), (ctypes.c_int * 1)(0)
    assert lib.hh_fusion_sum_forward_dt(2, ptrs, sh, 1, c.B, c.H, c.W, c.cin, 1, out.data_ptr(), None) == 1
    assert b"dtype" in lib.hh_last_error()
    assert lib.hh_bn_train_stats_dt(-1, x.data_ptr(), c.H * c.W, c.cin, out.data_ptr(), out.data_ptr(), None) == 1 and b"dtype" in lib.hh_last_error()


class _UnsuffixedABI:
    """the library with every `name_dt(HH_ACT_BF16, ...)` call routed to `name(...)`: what the ops called before the _dt family existed"""

    def __init__(self, lib):
        self._lib = lib
        self.routed = set()

    def __getattr__(self, name):
        if not name.endswith("_dt"):
            return getattr(self._lib, name)
        old = getattr(self._lib, name[:-3])

        def call(act_dtype, *args):
            assert act_dtype == 0, name
            self.routed.add(name)
            return old(*args)
        return call


def test_bf16_through_the_dt_entry_points_gives_the_bits_of_the_old_ones(pkg, monkeypatch):
    ops = _ops()
    lib = pkg._lib.load()
    conv_cases = [c for c in tbf.CONV_CASES if tbf.conv_id(c) in ("64to64-k3s1-3x16x24-p11", "48to96-k3s2-3x12x48-p11", "80to32-k2s1-3x3x17-p01", "48to64-k1s1-3x6x24-p00")]
    bn_cases = [c for c in tbf.BN_CASES if tbf.bn_id(c) in ("C48-3x24x24-res-relu", "C32-3x24x24-relu-special")]
    fu_cases = [c for c in tbf.FUSION_CASES if tbf.fusion_id(c) in ("C32-3x32x64-s0125-relu", "C48-1x8x24-s02")]
    assert len(conv_cases) == 4 and len(bn_cases) == 2 and len(fu_cases) == 2
    monkeypatch.setattr(ops, "_all_reduce_sums", lambda sums, group: None)
    BF = torch.bfloat16

    def run():
        out = []
        for c in conv_cases:
            i = {k: (tbf.bf(v).to(BF).float() if k != "bias" else v) for k, v in tbf.conv_inputs(c).items()}  # bf16-representable operands
            w = i["w"].to(DEV)
            pw = ops.PackedConvWeights([(w, c.stride, False), (w, c.stride, True)])
            pw.refresh()
            out += list(_conv_calls(ops, c, i, dtype=BF).values()) + list(_conv_calls(ops, c, i, packed=tuple(pw.buffers), dtype=BF).values()) + pw.buffers
        for c in bn_cases:
            i = tbf.bn_inputs(c)
            x, dy, res = _d(i["x"], BF), _d(i["dy"], BF), _d(i["res"], BF) if c.res else None
            gamma, beta = i["gamma"].to(DEV), i["beta"].to(DEV)
            y, mean, invstd = ops.bn_train_forward(x, gamma, beta, tbf.BN_EPS, res, c.relu)
            out += [y, mean, invstd, *ops.bn_train_backward(x, y, dy, mean, invstd, gamma, c.relu, want_dres=c.res)]
            if not c.res:
                out += list(ops.bn_train_backward(x, None, dy, mean, invstd, gamma, c.relu, beta=beta))
            ys, ms, iss, count = ops.sync_bn_train_forward(x, gamma, beta, tbf.BN_EPS, res, c.relu, None, 1)
            out += [ys, ms, iss, *ops.sync_bn_train_backward(x, ys, dy, ms, iss, gamma, c.relu, c.res, None, count)]
        for c in fu_cases:
            i = tbf.fusion_inputs(c)
            o = ops.fusion_sum([_d(t, BF) for t in i["terms"]], list(c.shifts), relu=c.relu)
            out += [o, *ops.fusion_sum_backward(_d(i["dy"], BF), o, list(c.shifts), relu=c.relu)]
        return [t for t in out if t is not None]

    new = run()
    old_abi = _UnsuffixedABI(lib)
    monkeypatch.setattr(pkg._lib, "load", lambda: old_abi)
    old = run()
    monkeypatch.undo()
    dt_names = {n for n in pkg._lib.exported_symbols() if n.endswith("_dt")}
    assert old_abi.routed == dt_names and len(dt_names) == 13, sorted(dt_names - old_abi.routed)
    assert len(new) == len(old) > 50
    for j, (a, b) in enumerate(zip(new, old)):
        _same(a, b, f"result {j}: _dt entry point with HH_ACT_BF16 vs the entry point without the suffix")


def test_report_worst_ratios(pkg):
    """(runs last in this file) the worst engine / allowed ratio per op family of this process, and the file's wall time"""
    print("worst engine / allowed: " + "; ".join(f"{k} {v:.3f}" for k, v in sorted(WORST.items())) + f"; wall time {time.time() - T0:.0f} s")
