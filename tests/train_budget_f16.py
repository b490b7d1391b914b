"""The error budgets of tests/train_budget.py for fp16 activations (a plain module, like train_budget.py).

The derivation is that module's; this one loads its source a second time under another module name and sets the second copy's format
constants, which its functions read when they are called:

  U16 = 2^-11          the unit roundoff of an fp16 store (11 significand bits; bf16: 2^-8)
  bf                   rounds through torch.float16
  K_SENSITIVE = 1.0    see below

and adds ETA = 2^-25, half the spacing of the fp16 subnormals, to every budget of an fp16-stored tensor:

  stored fp16 tensor                   allowed = u_h (|ref| + A) + A + ETA, u_h = 2^-11, A as derived in train_budget.py
  weight gradient (fp32), sensitive    K sqrt(n) u32 S with K = 1.0
  fp32 / fp64 quantities               (mean, invstd, dgamma, dbeta, the hard weight-gradient bound) unchanged

ETA.  Below 2^-14 an fp16 store no longer rounds relative to the value but to a multiple of 2^-24, so its error is up to 2^-25 whatever
|ref| is.  Without the term the CPU emulation of the BatchNorm dx reaches 2.7 x its budget on outputs below 2^-14; with it 0.996 x.
A tensor whose budget is zero because the kernel copies or masks (dres, the gradient of a same-resolution fusion term) gets no ETA.

K.  fp16 operands carry 11 significant bits, their products 22, so a short fp32 sum of them is no longer exact as it is for bf16
products (16 bits), and the two fp32 reference computations sit further from fp64.  measure_K() of the second copy (fp16-rounded
operands, seeds 0..5, (a) torch fp32 autograd and (b) sequential fp32; `python tests/train_budget_f16.py`): worst 0.893 at
48to96-k3s1-1x3x12-p11; worst over the lattice per seed 0..5: 0.634 0.893 0.652 0.683 0.682 0.718.  K = 1.0: the measured maximum
rounded up to the next half, as the bf16 module rounds.  Measured from the reference side only.

Overflow.  fp16 rounds a magnitude of 65520 or more to inf, and the kernels do not saturate (the loss scaler finds an oversized
scale by the inf).  check_f16 is train_budget.check with that rule in front: where |ref| - allowed >= 65520 the stored value must be
the inf of ref's sign, where |ref| + allowed < 65520 it must be finite and inside the budget, in between either is right.

Everything else -- the lattices, the references, the emulations, check -- is reached through this module as it is in the copy
(`tbf.CONV_CASES`, `tbf.conv_refs`, ...).
"""
from __future__ import annotations

import importlib.util
import os
import sys

import numpy as np
import torch

_spec = importlib.util.spec_from_file_location("train_budget_f16_copy", os.path.join(os.path.dirname(os.path.abspath(__file__)), "train_budget.py"))
_tb = importlib.util.module_from_spec(_spec)
sys.modules[_spec.name] = _tb
_spec.loader.exec_module(_tb)

ETA = 2.0 ** -25
F16_MAX, F16_OVER = 65504.0, 65520.0  # the largest finite fp16; the smallest magnitude round-to-nearest-even turns into inf
F16_MIN_NORMAL, F16_MIN_SUBNORMAL = 2.0 ** -14, 2.0 ** -24

_tb.U16 = 2.0 ** -11
_tb.K_SENSITIVE = 1.0
_tb.bf = lambda t: t.to(torch.float16).float()

# ---- ETA on every fp16-stored tensor.  The copy's functions find each other through its globals, so the replacements go there.
_stored0, _bn_fw0, _bn_bw0, _fu_fw0, _fu_bw0 = _tb._stored, _tb.bn_forward_refs, _tb.bn_backward_refs, _tb.fusion_forward_ref, _tb.fusion_backward_refs


def _stored(ref, n, S):
    return _stored0(ref, n, S) + ETA


def bn_forward_refs(c, seed: int = 0) -> dict:
    out = dict(_bn_fw0(c, seed))
    out["y"] = (out["y"][0], out["y"][1] + ETA)
    return out


def bn_backward_refs(c, y_kernel, seed: int = 0) -> dict:
    out = dict(_bn_bw0(c, y_kernel, seed))
    out["dx"] = (out["dx"][0], out["dx"][1] + ETA)
    return out


def fusion_forward_ref(c, seed: int = 0):
    ref, allowed = _fu_fw0(c, seed)
    return ref, allowed + ETA


def fusion_backward_refs(c, out_kernel, seed: int = 0) -> list:
    return [(r, a if s == 0 else a + ETA) for (r, a), s in zip(_fu_bw0(c, out_kernel, seed), c.shifts)]


for _f in (_stored, bn_forward_refs, bn_backward_refs, fusion_forward_ref, fusion_backward_refs):
    setattr(_tb, _f.__name__, _f)


def __getattr__(name):  # the rest of the copy: lattices, ids, references, emulations, check, U16 / U32 / U64 / K_SENSITIVE / bf
    return getattr(_tb, name)


def check_f16(got, ref, allowed, what: str, spatial: bool = True) -> float:
    """train_budget.check for an fp16-stored tensor that may overflow (the docstring's rule); -> the worst |err| / allowed of the
    elements that have to be finite"""
    got, ref, allowed = (np.array(t.detach().cpu().double().numpy() if isinstance(t, torch.Tensor) else t, np.float64) for t in (got, ref, allowed))
    must, may = np.abs(ref) - allowed >= F16_OVER, np.abs(ref) + allowed >= F16_OVER
    right_inf = np.isinf(got) & (np.sign(got) == np.sign(ref))
    ok_inf = may & right_inf
    got = np.where(must & ~right_inf, np.nan, np.where(ok_inf, 0.0, got))  # a finite value where inf is due: an infinite error
    ref = np.where(ok_inf, 0.0, ref)
    return _tb.check(got, ref, allowed, what, spatial)


# ---------------------------------------------------------------------------------------------------------------- special values
SPECIAL_CONV = _tb.ConvCase(32, 32, 3, 1, 1, 6, 16, (1, 1))  # one small case for overflow, inf / NaN and subnormals


def special_conv_inputs(kind: str, seed: int = 0) -> dict:
    """the operands of SPECIAL_CONV (conv_inputs' distribution), rescaled and rounded to fp16 again:
    "overflow"   x * 1024, w * 64: the forward's true values have a standard deviation near 9e4, so about half of the positive
                 ones lie beyond 65520
    "subnormal"  w, bias, res, gres * 2^-16: the weights (about 2^-20) and most outputs and data gradients are fp16 subnormals"""
    i = dict(_tb.conv_inputs(SPECIAL_CONV, seed))
    if kind == "overflow":
        i["x"], i["w"] = _tb.bf(i["x"] * 1024.0), _tb.bf(i["w"] * 64.0)
    elif kind == "subnormal":
        s = 2.0 ** -16
        i["w"], i["res"], i["gres"] = _tb.bf(i["w"] * s), _tb.bf(i["res"] * s), _tb.bf(i["gres"] * s)
        i["bias"] = _tb.bf(i["bias"] * s)
    else:
        raise ValueError(kind)
    return i


def special_conv_refs(i: dict) -> dict:
    """conv_refs for explicit operands: {fwd, dgrad, dgrad_res: (fp64 reference, allowed), wgrad: (reference, hard, sensitive)}"""
    c = SPECIAL_CONV
    d, a = _tb._cast(i, torch.float64), _tb._cast(i, torch.float64, True)
    fwd = _tb.conv_forward(d, c)
    out = {"fwd": (fwd, _stored(fwd, c.cin * c.ks * c.ks, _tb.conv_plain(a["x"], a["w"], c) + a["bias"].view(1, -1, 1, 1) + a["res"]))}
    dx, dw = _tb.conv_grads(d["x"], d["w"], d["dy"], c)
    sx, sw = _tb.conv_grads(a["x"], a["w"], a["dy"], c)
    n = c.cout * c.ks * c.ks
    out["dgrad"] = (dx, _stored(dx, n, sx))
    out["dgrad_res"] = (dx + d["gres"], _stored(dx + d["gres"], n, sx + a["gres"]))
    npix = c.B * c.H * c.W
    out["wgrad"] = (dw, (npix + 2) * _tb.U32 * sw, _tb.K_SENSITIVE * npix ** 0.5 * _tb.U32 * sw)
    return out


if __name__ == "__main__":
    import time
    torch.set_num_threads(16)
    t0 = time.time()
    res = _tb.measure_K(cases=[_tb.CONV_CASES[int(a)] for a in sys.argv[1:]] or None)
    for name, label in (("a", "(a) torch fp32 autograd"), ("b", "(b) sequential fp32")):
        top = max(res[name].items(), key=lambda kv: max(kv[1]))
        allmax = [max(v[s] for v in res[name].values()) for s in range(len(top[1]))]
        print(f"{label}: worst {max(top[1]):.3f} at {top[0]}; worst over the lattice per seed 0..5: " + " ".join(f"{v:.3f}" for v in allmax))
    print(f"{time.time() - t0:.0f} s")
