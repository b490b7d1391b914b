"""-m gpu: the training ops against fp64 references over the lattices of tests/train_budget.py, element by element within budgets derived
from the operands (that module's docstring).

hh_conv2d in its three modes (forward with bias + residual + ReLU, data gradient of a stride-1 / stride-2 conv with and without the
skip gradient), hh_conv2d_wgrad, the packed-weights path (bit-identical), train_net.conv / deconv_k4s2 with their channel padding, the
hh_bn_train_* family (fused, without y, and split around the exchange at world 1 and an emulated world 2) and hh_fusion_sum_*.  Every
call is repeated once for identical bits, and forward / data gradient of image b alone give the bits of slot b of the batch.

The library passes every case as it stands: no kernel or wrapper fix was needed.  Worst engine / allowed ratio per op family on the
MI355X (test_report_worst_ratios prints them; 1.0 = at the budget):
  conv forward 0.994   conv data gradient 0.995   BatchNorm forward 0.997   BatchNorm backward 0.998   fusion sum forward / backward 0.996
    (bf16-stored tensors: the store's own half ulp fills the budget, as it does for the CPU emulation, 0.985 .. 0.996)
  conv weight gradient: hard bound 0.051, sensitive bound 0.545 (K = 0.5, so 0.27 sqrt(n) u32 S: below the 0.33 the CPU computations reach;
    no sign of a truncating accumulator)
  train_net.conv / deconv_k4s2: output 0.972, data gradient 0.990, bias gradient 0.740, weight gradient hard 0.009, sensitive 0.228
Wall time of this file on an MI355X, fp64 references included: 11 s for its 141 tests.
"""
import importlib
import time

import pytest
import torch
import torch.nn.functional as F

import train_budget as tb
from conftest import PKG

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WORST = {}   # op family -> worst engine / allowed ratio of this process
T0 = time.time()


def _ops():
    return importlib.import_module(PKG + ".keypoints.train_ops")


def _d(t):
    """bf16 NHWC on the device (the values are bf16-representable already)"""
    return t.to(DEV, torch.bfloat16).contiguous(memory_format=torch.channels_last)


def _note(family, ratio):
    WORST[family] = max(WORST.get(family, 0.0), ratio)
    return round(ratio, 3)


def _same(a, b, what):
    assert a.shape == b.shape and torch.equal(a, b), f"{what}: {int((a != b).sum())} of {a.numel()} values differ"


# ---------------------------------------------------------------------------------------------------------------- convolutions
def _conv_calls(ops, c, i, packed=None):
    """the four calls of one case -> {fwd, dgrad, dgrad_res, wgrad}; packed: (forward, data-gradient) buffers of PackedConvWeights"""
    pad = c.pad if c.ks == 2 else None  # (3x3 and 1x1 take the default, as train_net does)
    x, dy, w = _d(i["x"]), _d(i["dy"]), i["w"].to(DEV)
    pf, pb = packed or (None, None)
    bias = i["bias"].to(DEV) if (packed is None or c.cout % 32 == 0) else None  # the packed call takes a bias of a multiple of 32 entries only
    out = {"fwd": ops.conv2d(x, w, c.stride, bias=bias, res=_d(i["res"]), relu=True, pad=pad, packed=pf),
           "dgrad": ops.conv2d(dy, w, c.stride, data_grad=True, pad=pad, packed=pb),
           "dgrad_res": ops.conv2d(dy, w, c.stride, data_grad=True, pad=pad, packed=pb, res=_d(i["gres"]))}
    if packed is None:
        out["wgrad"] = ops.conv2d_weight_grad(x, dy, c.ks, c.stride, pad=pad)
    elif bias is None:
        out["fwd_ref"] = ops.conv2d(x, w, c.stride, res=_d(i["res"]), relu=True, pad=pad)  # what the packed forward must equal
    return out


@pytest.mark.parametrize("case", tb.CONV_CASES, ids=tb.conv_id)
def test_conv_ops_vs_fp64_within_budget(pkg, case):
    ops, i, refs = _ops(), tb.conv_inputs(case), tb.conv_refs(case)
    got = _conv_calls(ops, case, i)
    again = _conv_calls(ops, case, i)
    for k in got:
        _same(again[k], got[k], f"{tb.conv_id(case)} {k}: second call vs first")
    ratios = {}
    for k, fam in (("fwd", "conv forward"), ("dgrad", "conv data gradient"), ("dgrad_res", "conv data gradient")):
        ratios[k] = _note(fam, tb.check(got[k].float().cpu(), *refs[k], f"{tb.conv_id(case)} {k}"))
    ref, hard, sens = refs["wgrad"]
    ratios["wgrad hard"] = _note("conv weight gradient (hard)", tb.check(got["wgrad"].cpu(), ref, hard, f"{tb.conv_id(case)} wgrad, hard bound", spatial=False))
    ratios["wgrad sensitive"] = _note("conv weight gradient (sensitive)",
                                      tb.check(got["wgrad"].cpu(), ref, sens, f"{tb.conv_id(case)} wgrad, sensitive bound", spatial=False))
    print(f"engine / allowed {tb.conv_id(case)}: {ratios}")


@pytest.mark.parametrize("case", tb.CONV_CASES, ids=tb.conv_id)
def test_conv_packed_weights_same_bits(pkg, case):
    ops, i = _ops(), tb.conv_inputs(case)
    w = i["w"].to(DEV)
    pw = ops.PackedConvWeights([(w, case.stride, False), (w, case.stride, True)])
    pw.refresh()
    plain, packed = _conv_calls(ops, case, i), _conv_calls(ops, case, i, packed=tuple(pw.buffers))
    _same(packed["fwd"], packed.get("fwd_ref", plain["fwd"]), f"{tb.conv_id(case)} packed forward")
    _same(packed["dgrad"], plain["dgrad"], f"{tb.conv_id(case)} packed data gradient")
    _same(packed["dgrad_res"], plain["dgrad_res"], f"{tb.conv_id(case)} packed data gradient with res")


@pytest.mark.parametrize("case", [c for c in tb.CONV_CASES if c.B > 1], ids=tb.conv_id)
def test_conv_images_of_a_batch_are_independent(pkg, case):
    ops, i = _ops(), tb.conv_inputs(case)
    batch = _conv_calls(ops, case, i)
    for b in range(case.B):
        one = _conv_calls(ops, case._replace(B=1), {k: (v[b:b + 1] if v.dim() == 4 and k != "w" else v) for k, v in i.items()})
        for k in ("fwd", "dgrad", "dgrad_res"):
            _same(batch[k][b:b + 1], one[k], f"{tb.conv_id(case)} {k}: slot {b} of the batch vs that image alone")


# ---------------------------------------------------------------------------------------------------------------- wrappers
def _wgrad_checks(got, ref, n, S, what):
    r = _note("wrapper weight gradient (hard)", tb.check(got, ref, (n + 2) * tb.U32 * S, what + ", hard bound", spatial=False))
    s = _note("wrapper weight gradient (sensitive)", tb.check(got, ref, tb.K_SENSITIVE * n ** 0.5 * tb.U32 * S, what + ", sensitive bound", spatial=False))
    return r, s


@pytest.mark.parametrize("cin,cout,ks,stride,shape", [(3, 64, 3, 2, (3, 12, 40)), (32, 17, 1, 1, (3, 6, 17)), (32, 34, 1, 1, (5, 3, 24)), (66, 32, 3, 1, (3, 6, 40))],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_train_net_conv_channel_padding(pkg, cin, cout, ks, stride, shape):
    """train_net.conv pads 3 -> 16, 17 -> 32, 34 -> 48, 66 -> 80 channels and slices the result back; the bias is a bf16 add behind the
    kernel.  Budgets: the conv's own, then one more bf16 rounding for the bias add; the gradients' are the ops' (padding and slicing
    copy); the bias gradient is a bf16-rounded fp32 sum."""
    tn = importlib.import_module(PKG + ".keypoints.train_net")
    B, H, W = shape
    g = torch.Generator().manual_seed(4000 + cin)
    m = torch.nn.Conv2d(cin, cout, ks, stride, (ks - 1) // 2, bias=True)
    with torch.no_grad():
        m.weight.copy_(tb.bf(torch.randn(m.weight.shape, generator=g) * (2.0 / (cin * ks * ks)) ** 0.5))
        m.bias.copy_(tb.bf(torch.randn(cout, generator=g)))
    x = tb.bf(torch.randn(B, cin, H, W, generator=g))
    dy = tb.bf(torch.randn(B, cout, H // stride, W // stride, generator=g))
    xr, wr, br = x.double().requires_grad_(), m.weight.detach().double().requires_grad_(), m.bias.detach().double().requires_grad_()
    r1 = F.conv2d(xr, wr, None, stride, (ks - 1) // 2)
    (r1 + br.view(1, -1, 1, 1)).backward(dy.double())
    xa, wa = x.double().abs().requires_grad_(), m.weight.detach().double().abs().requires_grad_()
    s1 = F.conv2d(xa, wa, None, stride, (ks - 1) // 2)
    s1.backward(dy.double().abs())
    m = m.to(DEV)
    xd = _d(x).requires_grad_()
    y = tn.conv(xd, m)
    y.backward(_d(dy))
    a1 = tb._stored(r1.detach(), cin * ks * ks, s1.detach())
    ref = (r1 + br.view(1, -1, 1, 1)).detach()
    what = f"train_net.conv {cin}->{cout} k{ks}s{stride}"
    ratios = {"y": _note("wrapper output", tb.check(y.detach().float().cpu(), ref, a1 + tb.U16 * (ref.abs() + a1), what + " output")),
              "dx": _note("wrapper data gradient", tb.check(xd.grad.float().cpu(), xr.grad, tb._stored(xr.grad, cout * ks * ks, xa.grad), what + " dx"))}
    n = dy.shape[0] * dy.shape[2] * dy.shape[3]
    ratios["dw"] = _wgrad_checks(m.weight.grad.cpu(), wr.grad, n, wa.grad, what + " dw")
    sb = dy.double().abs().sum((0, 2, 3))
    ratios["dbias"] = _note("wrapper bias gradient", tb.check(m.bias.grad.cpu(), br.grad, tb._stored(br.grad, n, sb), what + " dbias", spatial=False))
    print(f"engine / allowed {what}: {ratios}")


@pytest.mark.parametrize("cin,cout,shape", [(66, 32, (3, 3, 17)), (82, 48, (1, 6, 24))], ids=str)
def test_train_net_deconv_k4s2(pkg, cin, cout, shape):
    """ConvTranspose2d(k 4, s 2, p 1) as four 2x2 phase convs with asymmetric padding.  Output: each element is one phase conv's (n = 4 cin);
    dx: the four phases' data gradients, each rounded to bf16, added by autograd in bf16 (three more roundings); dw: every tap belongs to
    one phase, so the weight gradient is that phase's."""
    tn = importlib.import_module(PKG + ".keypoints.train_net")
    B, H, W = shape
    g = torch.Generator().manual_seed(5000 + cin)
    m = torch.nn.ConvTranspose2d(cin, cout, 4, 2, 1, bias=False)
    with torch.no_grad():
        m.weight.copy_(tb.bf(torch.randn(m.weight.shape, generator=g) * (2.0 / (cin * 4)) ** 0.5))
    x, dy = tb.bf(torch.randn(B, cin, H, W, generator=g)), tb.bf(torch.randn(B, cout, 2 * H, 2 * W, generator=g))

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
            a_p = tb._stored(r_p, cout * 4, s_p)
            a_dx, partial = a_dx + a_p, partial + r_p.abs() + a_p
    a_dx = a_dx + 3 * tb.U16 * partial
    m = m.to(DEV)
    xd = _d(x).requires_grad_()
    y = tn.deconv_k4s2(xd, m)
    y.backward(_d(dy))
    what = f"deconv_k4s2 {cin}->{cout} {shape}"
    ratios = {"y": _note("wrapper output", tb.check(y.detach().float().cpu(), ref, tb._stored(ref, cin * 4, S), what + " output")),
              "dx": _note("wrapper data gradient", tb.check(xd.grad.float().cpu(), dx, a_dx, what + " dx")),
              "dw": _wgrad_checks(m.weight.grad.cpu(), dw, B * H * W, sw, what + " dw")}
    print(f"engine / allowed {what}: {ratios}")


# ---------------------------------------------------------------------------------------------------------------- BatchNorm
@pytest.mark.parametrize("case", tb.BN_CASES, ids=tb.bn_id)
def test_batchnorm_ops_vs_fp64_within_budget(pkg, case, monkeypatch):
    ops, i, cid = _ops(), tb.bn_inputs(case), tb.bn_id(case)
    x, dy, res = _d(i["x"]), _d(i["dy"]), _d(i["res"]) if case.res else None
    gamma, beta = i["gamma"].to(DEV), i["beta"].to(DEV)
    fr = tb.bn_forward_refs(case)
    ratios = {}

    def forward_checks(y, mean, invstd, tag):
        for k, v, sp in (("mean", mean, False), ("invstd", invstd, False), ("y", y.float(), True)):
            ratios[tag + k] = _note("BatchNorm forward", tb.check(v.cpu(), *fr[k], f"{cid} {tag}{k}", spatial=sp))

    def backward_checks(out, br, tag):
        for k, v in zip(("dx", "dgamma", "dbeta", "dres"), out):
            if k in br:
                ratios[tag + k] = _note("BatchNorm backward", tb.check(v.float().cpu(), *br[k], f"{cid} {tag}{k}", spatial=k in ("dx", "dres")))
            else:
                assert v is None

    y, mean, invstd = ops.bn_train_forward(x, gamma, beta, tb.BN_EPS, res, case.relu)
    y2, mean2, invstd2 = ops.bn_train_forward(x, gamma, beta, tb.BN_EPS, res, case.relu)
    _same(y2, y, f"{cid} y: second call vs first"); _same(mean2, mean, f"{cid} mean again"); _same(invstd2, invstd, f"{cid} invstd again")
    forward_checks(y, mean, invstd, "")
    br = tb.bn_backward_refs(case, y.float())
    out = ops.bn_train_backward(x, y, dy, mean, invstd, gamma, case.relu, want_dres=case.res)
    backward_checks(out, br, "")
    for a, b in zip(ops.bn_train_backward(x, y, dy, mean, invstd, gamma, case.relu, want_dres=case.res), out):
        assert (a is None and b is None) or torch.equal(a, b), f"{cid} backward: second call vs first"
    if not case.res:  # without a residual the backward can do without y: the same bits
        plain = ops.bn_train_backward(x, None, dy, mean, invstd, gamma, case.relu, beta=beta)
        for k, a, b in zip(("dx", "dgamma", "dbeta"), plain, out):
            _same(a, b, f"{cid} backward without y, {k}")
    # the split entry points: world 1 (no exchange) and an emulated world 2 (every sum doubled = the batch concatenated with itself, whose
    # mean, variance, dx and per-rank dgamma / dbeta are those of the batch)
    for world in (1, 2):
        monkeypatch.setattr(ops, "_all_reduce_sums", (lambda sums, group: None) if world == 1 else (lambda sums, group: sums.mul_(2)))
        ys, ms, iss, count = ops.sync_bn_train_forward(x, gamma, beta, tb.BN_EPS, res, case.relu, None, world)
        assert count == world * case.B * case.H * case.W
        forward_checks(ys, ms, iss, f"world{world} ")
        brs = br if torch.equal(ys, y) else tb.bn_backward_refs(case, ys.float())
        backward_checks(ops.sync_bn_train_backward(x, ys, dy, ms, iss, gamma, case.relu, case.res, None, count), brs, f"world{world} ")
    print(f"engine / allowed {cid}: {ratios}")


# ---------------------------------------------------------------------------------------------------------------- fusion sum
@pytest.mark.parametrize("case", tb.FUSION_CASES, ids=tb.fusion_id)
def test_fusion_sum_vs_fp64_within_budget(pkg, case):
    ops, i, cid = _ops(), tb.fusion_inputs(case), tb.fusion_id(case)
    terms, dy, shifts = [_d(t) for t in i["terms"]], _d(i["dy"]), list(case.shifts)
    out = ops.fusion_sum(terms, shifts, relu=case.relu)
    _same(ops.fusion_sum(terms, shifts, relu=case.relu), out, f"{cid} out: second call vs first")
    ratios = [_note("fusion sum forward", tb.check(out.float().cpu(), *tb.fusion_forward_ref(case), f"{cid} out"))]
    grads = ops.fusion_sum_backward(dy, out, shifts, relu=case.relu)
    again = ops.fusion_sum_backward(dy, out, shifts, relu=case.relu)
    assert len(grads) == len(shifts)
    for j, (gj, rj) in enumerate(zip(grads, tb.fusion_backward_refs(case, out.float()))):
        _same(again[j], gj, f"{cid} gradient of term {j}: second call vs first")
        ratios.append(_note("fusion sum backward", tb.check(gj.float().cpu(), *rj, f"{cid} gradient of term {j} (shift {shifts[j]})")))
        if not case.relu and shifts[j] == 0:
            assert gj.data_ptr() == dy.data_ptr(), f"{cid}: without ReLU the gradient of a same-resolution term is dy itself"
    print(f"engine / allowed {cid}: {ratios}")


def test_report_worst_ratios(pkg):
    """(runs last in this file) the worst engine / allowed ratio per op family of this process, and the file's wall time"""
    print("worst engine / allowed: " + "; ".join(f"{k} {v:.3f}" for k, v in sorted(WORST.items())) + f"; wall time {time.time() - T0:.0f} s")
