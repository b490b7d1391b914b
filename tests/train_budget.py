"""Per-element error budgets for the training ops, derived from the operands alone (a plain module, like forward_budget.py).

Every reference is fp64 on the CPU from the bf16-rounded operands the kernel gets.  Every budget is a bound on what the kernel's
number formats can lose, built from the unit roundoffs u16 = 2^-8 (bf16 store) and u32 = 2^-24 (fp32 arithmetic) and from the same
operation on absolute values; nothing in it is measured on the engine.

  conv output, data gradient (bf16)   A = (n + 2) u32 S, allowed = u16 (|ref| + A) + A; n = products per output, S = the operation on
                                      |x|, |w| with |bias| and |res| added
  weight gradient (fp32), hard        (n + 2) u32 S, n = B Ho Wo, S = the weight gradient of |x|, |dy|: any summation order, never fails
  weight gradient (fp32), sensitive   K sqrt(n) u32 S: the hard bound is blind at large n (at n = 65536 a dropped 4 x 32 tile of one
                                      image stays below 0.29 of it, and puts 98 % of the elements over the sensitive one, up to 149 x)
  BatchNorm mean                      u32 |m| + P u64 mean|x|                      (fp32 rounding of a double sum; u64 = 2^-53)
  BatchNorm invstd                    invstd (u32 + dv / (2 (var + eps))), dv = (P + 4) u64 (mean x^2 + m^2): the double sums and the
                                      cancellation of b / P - m^2, which is what a mean-dominated channel magnifies
  BatchNorm y, dx (bf16)              u16 (|ref| + A) + A, A = first-order propagation of the errors of mean and invstd through the
                                      formula plus u32 per fp32 operation of bn_affine / the dx formula, each on absolute values
                                      (bn_forward_refs / bn_backward_refs spell the terms out); dres is exact (a masked copy of dy)
  BatchNorm dgamma, dbeta (fp32)      u32 |ref| + the double sum's P u64 sum|g|, dgamma plus sum|g| x the error of the fp32 xhat
  fusion sum (bf16)                   u16 |ref| + (terms - 1) u32 sum|term|; an up-term gradient the same with 4^shift addends; the
                                      gradient of the same-resolution terms is exact

K.  measure_K() (python tests/train_budget.py) takes the worst |err| / (sqrt(n) u32 S) over every element of every weight gradient of
CONV_CASES, seeds 0..5, of two fp32 CPU computations from the same operands: (a) torch fp32 autograd and (b) a strictly sequential
fp32 accumulation over the pixels in raster order, the longest chain any order has.  Measured (about a minute for all):
  (a) torch fp32 autograd: worst 0.331 at 96to192-k3s2-3x2x32-p11; worst over the lattice per seed 0..5: 0.309 0.307 0.286 0.304 0.331 0.250
  (b) sequential fp32:     worst 0.331 at 96to192-k3s2-3x2x32-p11; worst over the lattice per seed 0..5: 0.309 0.307 0.286 0.304 0.331 0.250
The worst sits at the smallest n (48 pixels): the last rounding of a sum alone, up to u32 |ref| <= u32 S, is 1 / sqrt(48) = 0.144 of the
unit there and the chain adds the rest; the two orders agree because torch sums so few pixels in one chain too.  On the n = 65536 case
(`python tests/train_budget.py 6`: the arguments are indices into CONV_CASES) (a) is at 0.002 and (b) at 0.018 (seeds 0..5: 0.012 0.012
0.013 0.016 0.017 0.018).  K = 0.5: the measured maximum rounded up to the next half, as forward_budget.py rounds its margins.

The emulation of test_train_budget_cpu.py (torch fp32, bf16 where the kernel stores bf16) stays inside every budget on every case; the
planted defects of that file are all flagged.  Wall time of that file: 15 s for its 72 tests on 8 threads;
tests/test_gpu_train_lattice.py carries the engine's ratios and its own wall time.
"""
from __future__ import annotations

import functools
import math
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

U16, U32, U64 = 2.0 ** -8, 2.0 ** -24, 2.0 ** -53
K_SENSITIVE = 0.5  # see the docstring: measured from the reference side only


def bf(t: torch.Tensor) -> torch.Tensor:
    """round to bf16 and back: the values the kernels see"""
    return t.to(torch.bfloat16).float()


# ---------------------------------------------------------------------------------------------------------------- lattices
ConvCase = namedtuple("ConvCase", "cin cout ks stride B H W pad")  # H, W: the conv's input; pad = (pad_y, pad_x) top / left
BNCase = namedtuple("BNCase", "C B H W res relu special")           # special: channels 0..2 are mean-dominated / constant / zero pre-activation
FusionCase = namedtuple("FusionCase", "C B H W shifts relu")

# instantiation numbers: the rows of CONV_CONFIGS (conv_mfma.hip); wgrad: tiles / workers of conv_wgrad_num_workers as it stands
CONV_CASES = [
    # -- the weight gradient's persistent loop: more tiles than workers, unevenly split (some workers run one tile more)
    ConvCase(256, 256, 3, 1, 5, 32, 32, (1, 1)),    # 3x3: 40 tiles / 32 workers; config 1 forward and data gradient
    ConvCase(32, 32, 3, 1, 3, 128, 96, (1, 1)),     # 3x3 small-channel: 288 / 256; config 0; non-square (tall)
    ConvCase(64, 256, 1, 1, 3, 64, 64, (0, 0)),     # 1x1: 96 / 64; config 9
    ConvCase(64, 128, 3, 2, 3, 128, 128, (1, 1)),   # 3x3 s2: 192 / 128; config 5, data gradient config 16
    ConvCase(80, 32, 2, 1, 5, 64, 64, (1, 1)),      # 2x2: 160 / 128; the W32 deconv head after padding (66 -> 80); config 15
    ConvCase(128, 128, 3, 1, 5, 64, 16, (1, 1)),    # 3x3 narrow: 80 / 64; config 2; width 16
    ConvCase(32, 32, 3, 1, 4, 128, 128, (1, 1)),    # n = 65536 pixels: where only the sensitive weight-gradient bound sees a dropped tile
    # -- instantiations no op-level test reached (3, 5, 6, 10, 12, 13, 14) and the tile-width fallbacks
    ConvCase(48, 96, 3, 1, 3, 6, 40, (1, 1)),       # 3x3 KC16 / NT1: config 3; height 6 (not a multiple of any tile height), width 40
    ConvCase(48, 96, 3, 1, 1, 3, 12, (1, 1)),       # the same on a narrow map: falls back to the 32-column config 3; height 3, width 12, batch 1
    ConvCase(48, 48, 3, 1, 3, 24, 40, (1, 1)),      # 3x3 KC16 / NT2 on a wide map: falls back to the 16-column config 4
    ConvCase(48, 48, 3, 1, 5, 2, 16, (1, 1)),       # config 4 as chosen; height 2, batch 5
    ConvCase(96, 48, 3, 1, 3, 17, 24, (1, 1)),      # data gradient reaches config 3 (48 in, 96 out); odd height 17, width 24
    ConvCase(32, 32, 3, 1, 3, 40, 12, (1, 1)),      # 3x3 KC32 / NT1 on a narrow map: falls back to config 0; weight gradient narrow, 32 channels
    ConvCase(16, 64, 3, 2, 3, 12, 80, (1, 1)),      # the stem's 16 -> 64 s2: config 5 (wide, 40 columns), data gradient config 15; 6 output rows
    ConvCase(16, 64, 3, 2, 1, 4, 24, (1, 1)),       # config 7 (narrow): 2 output rows of 12
    ConvCase(48, 96, 3, 2, 3, 12, 48, (1, 1)),      # W48 transition: config 6 (Cout tile 32, 24 columns), data gradient config 16
    ConvCase(48, 96, 3, 2, 5, 6, 34, (1, 1)),       # config 8 (narrow); 3 output rows of 17
    ConvCase(96, 192, 3, 2, 3, 2, 32, (1, 1)),      # W48 transition: a one-row output map, 16 columns
    ConvCase(192, 384, 3, 2, 1, 16, 48, (1, 1)),    # W48 transition, 24 channel blocks in the weight gradient
    ConvCase(32, 32, 1, 1, 3, 24, 40, (0, 0)),      # 1x1 Cout tile 32: config 10 forward and data gradient
    ConvCase(32, 32, 1, 1, 5, 6, 16, (0, 0)),       # the same narrow: config 12
    ConvCase(128, 64, 1, 1, 3, 3, 16, (0, 0)),      # 1x1 narrow, Cout tile 64: config 11 both ways
    ConvCase(48, 64, 1, 1, 3, 6, 24, (0, 0)),       # 1x1 KC16 / NT2: config 13
    ConvCase(48, 64, 1, 1, 1, 2, 12, (0, 0)),       # the same narrow: falls back to config 13
    ConvCase(64, 48, 1, 1, 3, 17, 40, (0, 0)),      # data gradient reaches config 13 (48 in, 64 out)
    ConvCase(32, 48, 1, 1, 3, 40, 17, (0, 0)),      # W48 fusion 1x1: config 9, data gradient config 14; wide (17 columns), tall
    ConvCase(48, 32, 1, 1, 3, 12, 40, (0, 0)),      # W48 fusion 1x1: config 14, data gradient config 9
    ConvCase(48, 32, 1, 1, 5, 1, 16, (0, 0)),       # narrow: falls back to config 14; a one-row map
    # -- the 2x2 phase convs of deconv_k4s2: every (pad_y, pad_x), forward, mode-1 data gradient (pad flipped) and weight gradient
    ConvCase(80, 32, 2, 1, 3, 6, 40, (0, 0)),
    ConvCase(80, 32, 2, 1, 3, 3, 17, (0, 1)),       # height 3, odd width 17
    ConvCase(80, 32, 2, 1, 1, 17, 24, (1, 0)),
    ConvCase(80, 32, 2, 1, 3, 2, 12, (1, 1)),       # narrow: falls back to config 15
    ConvCase(96, 48, 2, 1, 3, 6, 24, (0, 1)),       # the W48 head after padding (82 -> 96): config 16 (Cout tile 64)
    ConvCase(96, 48, 2, 1, 5, 3, 16, (1, 0)),       # narrow: falls back to config 16
    ConvCase(64, 32, 2, 1, 3, 12, 24, (0, 0)),      # data gradient reaches config 16 (32 in, 64 out)
    # -- the shapes of the older op-level test that stay interesting here: stride 2 from 32 channels, 16-row maps
    ConvCase(32, 32, 3, 2, 3, 24, 24, (1, 1)),      # config 8, data gradient config 15 narrow
    ConvCase(64, 64, 3, 1, 3, 16, 24, (1, 1)),      # config 1; wide and low
    ConvCase(32, 32, 3, 1, 1, 17, 40, (1, 1)),      # the small-channel weight gradient with one tile per worker (10 tiles); 17 rows of 40
]
WGRAD_N65536 = CONV_CASES[6]

BN_CASES = [
    BNCase(8, 3, 24, 24, False, True, False),      # C = 8: 256 pixel lanes per block
    BNCase(8, 1, 1, 2, True, True, False),         # P = 2: more pixel lanes than pixels
    BNCase(16, 1, 1, 97, False, False, False),     # P = 97 (prime)
    BNCase(16, 3, 24, 24, True, True, False),
    BNCase(32, 3, 24, 24, False, True, True),      # the special channels: mean = 50 std, constant, pre-activation exactly 0
    BNCase(32, 1, 97, 1, True, False, True),       # the special channels at a prime P, no ReLU
    BNCase(32, 2, 160, 160, False, True, False),   # P = 51200 > 49152: the four-pixel unrolled loop of bn_partial_kernel runs
    BNCase(48, 3, 24, 24, True, True, False),
    BNCase(64, 3, 24, 24, False, False, False),
    BNCase(96, 3, 24, 24, True, False, False),     # C / 8 = 12 does not divide 256: four idle threads per block
    BNCase(96, 1, 2, 1, False, True, False),       # P = 2
    BNCase(96, 2, 304, 304, True, True, False),    # P C / 8 / 256 = 8664 > 8192: the grid cap of the apply kernels
    BNCase(192, 3, 24, 24, False, True, False),
    BNCase(256, 3, 24, 24, True, True, False),
    BNCase(384, 1, 1, 97, False, True, False),
    BNCase(384, 3, 24, 24, True, False, False),
    BNCase(2048, 3, 24, 24, False, True, False),   # one pixel lane per block
    BNCase(2048, 1, 1, 2, True, True, False),      # P = 2 at the widest C
]
BN_EPS = float(np.float32(1e-5))  # the C-ABI takes eps as a float: the value the kernels add

FUSION_CASES = [
    FusionCase(32, 3, 32, 64, (0, 1, 2, 5), True),    # shift 5: a 1 x 2 term
    FusionCase(32, 1, 32, 32, (0, 5), False),         # relu off: the backward returns dy itself
    FusionCase(8, 3, 16, 48, (0, 4, 3), True),        # C = 8, shifts in descending order, odd batch
    FusionCase(8, 5, 4, 4, (0,), True),               # one term
    FusionCase(48, 3, 16, 16, (0, 0, 1, 4), True),    # W48, two same-resolution terms
    FusionCase(48, 1, 8, 24, (0, 2), False),
    FusionCase(128, 5, 8, 8, (0, 0, 0, 3), False),    # three same-resolution terms, relu off
    FusionCase(128, 3, 4, 12, (0, 1, 2), True),
]


def conv_id(c) -> str:
    return f"{c.cin}to{c.cout}-k{c.ks}s{c.stride}-{c.B}x{c.H}x{c.W}-p{c.pad[0]}{c.pad[1]}"


def bn_id(c) -> str:
    return f"C{c.C}-{c.B}x{c.H}x{c.W}" + ("-res" if c.res else "") + ("-relu" if c.relu else "") + ("-special" if c.special else "")


def fusion_id(c) -> str:
    return f"C{c.C}-{c.B}x{c.H}x{c.W}-s" + "".join(map(str, c.shifts)) + ("-relu" if c.relu else "")


# ---------------------------------------------------------------------------------------------------------------- check
def check(got, ref, allowed, what: str, spatial: bool = True) -> float:
    """asserts |got - ref| <= allowed element by element; -> the worst |err| / allowed.  A NaN counts as an infinite error.  spatial:
    the tensor is [B, C, H, W], and the offenders are split into border (first / last row or column, last image) and interior; other
    tensors (weight gradients, per-channel vectors) count as interior throughout."""
    got, ref, allowed = (np.asarray(t.detach().cpu().double() if isinstance(t, torch.Tensor) else t, np.float64) for t in (got, ref, allowed))
    assert got.shape == ref.shape == allowed.shape, (what, got.shape, ref.shape, allowed.shape)
    err = np.abs(got - ref)
    err = np.where(np.isfinite(err), err, np.inf)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err > 0, err / allowed, 0.0)  # err > 0 at allowed = 0: inf
    over = ~(err <= allowed)
    if over.any():
        idx = np.argwhere(over)
        at = np.unravel_index(np.argmax(np.where(over, ratio, -1.0)), ratio.shape)
        if spatial and got.ndim == 4:
            B, _, H, W = got.shape
            border = (idx[:, 0] == B - 1) | (idx[:, 2] == 0) | (idx[:, 2] == H - 1) | (idx[:, 3] == 0) | (idx[:, 3] == W - 1)
        else:
            border = np.zeros(len(idx), bool)
        parts = []
        for name, sel in (("border", border), ("interior", ~border)):
            parts.append(f"{name} {int(sel.sum())}" + (f" in {idx[sel].min(0).tolist()} .. {idx[sel].max(0).tolist()}" if sel.any() else ""))
        raise AssertionError(f"{what}: {len(idx)} of {over.size} elements over budget ({'; '.join(parts)}); worst at {[int(v) for v in at]}: "
                             f"{got[at]!r} vs {ref[at]!r}, |err| {err[at]:.4g} = {ratio[at]:.3g} x allowed {allowed[at]:.4g}")
    return float(ratio.max()) if ratio.size else 0.0


# ---------------------------------------------------------------------------------------------------------------- convolutions
def conv_out_hw(c):
    return (c.H // 2, c.W // 2) if c.stride == 2 else (c.H, c.W)


@functools.lru_cache(maxsize=None)
def conv_inputs(c: ConvCase, seed: int = 0) -> dict:
    """bf16-rounded fp32 operands: x, w, dy, res (forward residual), gres (the skip gradient of the data gradient); bias fp32"""
    g = torch.Generator().manual_seed(1000 * seed + CONV_CASES.index(c) if c in CONV_CASES else seed)
    Ho, Wo = conv_out_hw(c)
    return {
        "x": bf(torch.randn(c.B, c.cin, c.H, c.W, generator=g)),
        "w": bf(torch.randn(c.cout, c.cin, c.ks, c.ks, generator=g) * (2.0 / (c.cin * c.ks * c.ks)) ** 0.5),
        "bias": torch.randn(c.cout, generator=g),
        "res": bf(torch.randn(c.B, c.cout, Ho, Wo, generator=g)),
        "dy": bf(torch.randn(c.B, c.cout, Ho, Wo, generator=g)),
        "gres": bf(torch.randn(c.B, c.cin, c.H, c.W, generator=g)),
    }


def conv_plain(x, w, c, pad=None):
    """conv(x, w) of case c with explicit top / left padding (bottom / right: what keeps the size at stride 1), any dtype"""
    py, px = c.pad if pad is None else pad
    return F.conv2d(F.pad(x, (px, c.ks - 1 - px, py, c.ks - 1 - py)), w, None, c.stride)


def conv_forward(i: dict, c, pad=None):
    return F.relu(conv_plain(i["x"], i["w"], c, pad) + i["bias"].to(i["x"].dtype).view(1, -1, 1, 1) + i["res"])


def conv_grads(x, w, dy, c, pad=None):
    """-> (dL/dx, dL/dw) by autograd of conv_plain"""
    x, w = x.detach().clone().requires_grad_(), w.detach().clone().requires_grad_()
    conv_plain(x, w, c, pad).backward(dy)
    return x.grad, w.grad


def _cast(i: dict, dtype, absolute=False) -> dict:
    return {k: (v.abs() if absolute else v).to(dtype) for k, v in i.items()}


def _stored(ref, n, S):
    A = (n + 2) * U32 * S
    return U16 * (ref.abs() + A) + A


@functools.lru_cache(maxsize=None)
def conv_refs(c: ConvCase, seed: int = 0) -> dict:
    """{tensor: (fp64 reference, allowed)} for fwd, dgrad, dgrad_res, and wgrad: (reference, hard bound, sensitive bound)"""
    i = conv_inputs(c, seed)
    d, a = _cast(i, torch.float64), _cast(i, torch.float64, True)
    Ho, Wo = conv_out_hw(c)
    fwd = conv_forward(d, c)
    out = {"fwd": (fwd, _stored(fwd, c.cin * c.ks * c.ks, conv_plain(a["x"], a["w"], c) + a["bias"].view(1, -1, 1, 1) + a["res"]))}
    dx, dw = conv_grads(d["x"], d["w"], d["dy"], c)
    sx, sw = conv_grads(a["x"], a["w"], a["dy"], c)
    n = c.cout * c.ks * c.ks
    out["dgrad"] = (dx, _stored(dx, n, sx))
    out["dgrad_res"] = (dx + d["gres"], _stored(dx + d["gres"], n, sx + a["gres"]))
    npix = c.B * Ho * Wo
    out["wgrad"] = (dw, (npix + 2) * U32 * sw, K_SENSITIVE * math.sqrt(npix) * U32 * sw)
    return out


def emulate_conv(i: dict, c, pad_fwd=None, pad_dgrad=None, pad_wgrad=None) -> dict:
    """the kernels' arithmetic on the CPU: torch fp32 on the same operands, bf16 where the kernel stores bf16 (the pads are there for
    the planted defects)"""
    dx, _ = conv_grads(i["x"], i["w"], i["dy"], c, pad_dgrad)
    _, dw = conv_grads(i["x"], i["w"], i["dy"], c, pad_wgrad)
    return {"fwd": bf(conv_forward(i, c, pad_fwd)), "dgrad": bf(dx), "dgrad_res": bf(dx + i["gres"]), "wgrad": dw}


def wgrad_sequential(i: dict, c) -> torch.Tensor:
    """the weight gradient as ONE fp32 accumulator per element that takes the pixels in raster order, image after image"""
    py, px = c.pad
    xp = F.pad(i["x"], (px, c.ks - 1 - px, py, c.ks - 1 - py))
    cols = F.unfold(xp, c.ks, stride=c.stride)          # [B, cin ks ks, Ho Wo]
    dy = i["dy"].flatten(2)                              # [B, cout, Ho Wo]
    acc = torch.zeros(c.cout, cols.shape[1])
    colsT, dyT = cols.transpose(1, 2).contiguous(), dy.transpose(1, 2).contiguous()
    for b in range(c.B):
        for p in range(colsT.shape[1]):
            acc.addr_(dyT[b, p], colsT[b, p])
    return acc.view(c.cout, c.cin, c.ks, c.ks)


def measure_K(seeds=(0, 1, 2, 3, 4, 5), cases=None):
    """-> {(a) / (b): (worst |err| / (sqrt(n) u32 S), case, per-seed worst)} over the weight gradients of the lattice"""
    worst = {}
    for c in cases or CONV_CASES:
        for s in seeds:
            i = conv_inputs(c, s)
            ref, _, sens = conv_refs(c, s)["wgrad"]
            unit = sens / K_SENSITIVE
            for name, got in (("a", conv_grads(i["x"], i["w"], i["dy"], c)[1]), ("b", wgrad_sequential(i, c))):
                r = float(((got.double() - ref).abs() / unit.clamp_min(1e-300)).max())
                worst.setdefault(name, {}).setdefault(conv_id(c), []).append(r)
            conv_refs.cache_clear()
            conv_inputs.cache_clear()
    return worst


# ---------------------------------------------------------------------------------------------------------------- BatchNorm
@functools.lru_cache(maxsize=2)
def bn_inputs(c: BNCase, seed: int = 0) -> dict:
    g = torch.Generator().manual_seed(2000 + 1000 * seed + BN_CASES.index(c) if c in BN_CASES else seed)
    shape = (c.B, c.C, c.H, c.W)
    P = c.B * c.H * c.W
    x = torch.randn(shape, generator=g) * 2 + 0.5
    gamma, beta = torch.rand(c.C, generator=g) + 0.5, torch.randn(c.C, generator=g) * 0.1
    if c.special:
        x[:, 0] = x[:, 0] / 2 + 50.0   # mean = 50 std: b / P - m^2 cancels four digits
        x[:, 1] = 100.5                # constant: the variance is 0, invstd = 1 / sqrt(eps)
        k = (P // 3) * 2               # as many +1.5 as -1.5 and zeros behind them: the mean is exactly 0 and x - mean = 0 at the zeros
        v = torch.zeros(P)
        v[0:k:2], v[1:k:2] = 1.5, -1.5
        x[:, 2] = v.view(c.B, c.H, c.W)
        beta[2] = 0.0
    return {"x": bf(x), "gamma": gamma, "beta": beta, "res": bf(torch.randn(shape, generator=g)) if c.res else None,
            "dy": bf(torch.randn(shape, generator=g))}


def _ch(v):
    return v.view(1, -1, 1, 1)


@functools.lru_cache(maxsize=2)
def bn_forward_refs(c: BNCase, seed: int = 0) -> dict:
    """{mean, invstd, y: (fp64 reference, allowed)}"""
    i = bn_inputs(c, seed)
    x, gamma, beta = i["x"].double(), i["gamma"].double(), i["beta"].double()
    P = c.B * c.H * c.W
    m = x.mean((0, 2, 3))
    xc = x - _ch(m)
    var = (xc * xc).mean((0, 2, 3))
    istd = (var + BN_EPS).rsqrt()
    a_m = U32 * m.abs() + P * U64 * x.abs().mean((0, 2, 3))
    dv = (P + 4) * U64 * ((x * x).mean((0, 2, 3)) + m * m)
    a_is = istd * (U32 + dv / (2 * (var + BN_EPS))) * (1 + 1e-6)
    t = xc * _ch(istd * gamma) + _ch(beta)
    if c.res:
        t = t + i["res"].double()
    y = F.relu(t) if c.relu else t
    T = xc.abs() * _ch(istd * gamma.abs())  # |gamma (x - mean) invstd|
    # errors of mean and invstd pushed through; x - mean, * invstd, * gamma: 3 u32 T; + beta, + res: u32 on each partial sum
    A = _ch(gamma.abs() * istd * a_m) + T * _ch(a_is / istd) + 3 * U32 * T + 2 * U32 * (T + _ch(beta.abs()) + (i["res"].double().abs() if c.res else 0))
    return {"mean": (m, a_m), "invstd": (istd, a_is), "y": (y, U16 * (y.abs() + A) + A)}


def bn_backward_refs(c: BNCase, y_kernel: torch.Tensor, seed: int = 0) -> dict:
    """{dx, dgamma, dbeta, dres: (fp64 reference, allowed)}; the ReLU mask is y_kernel > 0: the kernel's own bf16 output"""
    i = bn_inputs(c, seed)
    x, gamma = i["x"].double(), i["gamma"].double()
    P = c.B * c.H * c.W
    fw = bn_forward_refs(c, seed)
    (m, a_m), (istd, a_is) = fw["mean"], fw["invstd"]
    g = i["dy"].double()
    if c.relu:
        g = g * (y_kernel.detach().cpu().double() > 0)
    xh = (x - _ch(m)) * _ch(istd)
    a_xh = _ch(istd * a_m) + (x - _ch(m)).abs() * _ch(a_is) + 2 * U32 * xh.abs()  # the fp32 xhat of the kernels
    dbeta, dgamma = g.sum((0, 2, 3)), (g * xh).sum((0, 2, 3))
    sg = g.abs().sum((0, 2, 3))
    a_db = U32 * dbeta.abs() + P * U64 * sg
    a_dg = U32 * dgamma.abs() + (g.abs() * a_xh).sum((0, 2, 3)) + P * U64 * (g * xh).abs().sum((0, 2, 3))
    t2, t3 = _ch(dbeta / P), xh * _ch(dgamma / P)
    inner = g - t2 - t3
    dx = _ch(gamma * istd) * inner
    a_inner = (3 * U32 * t2.abs() + _ch(a_db / P) + 4 * U32 * t3.abs() + _ch(dgamma.abs() / P) * a_xh + xh.abs() * _ch(a_dg / P)
               + 2 * U32 * (g.abs() + t2.abs() + t3.abs()))
    A = _ch(gamma.abs() * istd) * a_inner + dx.abs() * (3 * U32 + _ch(a_is / istd))
    out = {"dx": (dx, U16 * (dx.abs() + A) + A), "dgamma": (dgamma, a_dg), "dbeta": (dbeta, a_db)}
    if c.res:
        out["dres"] = (g, torch.zeros_like(g))
    return out


def emulate_bn_forward(i: dict, c, unbiased=False, fp32_var=None) -> dict:
    """the kernels' arithmetic: double sums, mean / invstd rounded to fp32, bn_affine in fp32, bf16 store.  The flags are planted defects;
    fp32_var = "clamped" / "unclamped": the sums and b / P - m^2 in fp32 (one accumulator each, pixel after pixel), where the
    cancellation of a constant channel leaves rounding noise of either sign, with and without the clamp at 0"""
    x = i["x"]
    P = c.B * c.H * c.W
    a, b = x.double().sum((0, 2, 3)), (x.double() ** 2).sum((0, 2, 3))
    m = a / P
    var = b / P - m * m
    var = var.clamp_min(0)
    if unbiased:
        var = var * P / max(P - 1, 1)
    istd = (1.0 / (var + BN_EPS).sqrt()).float()
    if fp32_var:
        xf = x.transpose(0, 1).flatten(1)
        a32, b32 = torch.zeros(c.C), torch.zeros(c.C)
        for p in range(P):
            a32, b32 = a32 + xf[:, p], b32 + xf[:, p] * xf[:, p]
        var32 = b32 / P - (a32 / P) ** 2
        if fp32_var == "clamped":
            var32 = var32.clamp_min(0)
        istd = (1.0 / (var32.double() + BN_EPS).sqrt()).float()
    m = m.float()
    t = (x - _ch(m)) * _ch(istd) * _ch(i["gamma"]) + _ch(i["beta"])
    if c.res:
        t = t + i["res"]
    return {"mean": m, "invstd": istd, "y": bf(F.relu(t) if c.relu else t)}


def emulate_bn_backward(i: dict, c, fw: dict, no_dgamma_term=False, dbeta_pm1=False, no_mask=False) -> dict:
    x, P = i["x"], c.B * c.H * c.W
    m, istd = fw["mean"], fw["invstd"]
    g = i["dy"]
    if c.relu and not no_mask:
        g = g * (fw["y"] > 0)
    xh = (x - _ch(m)) * _ch(istd)
    dbeta, dgamma = g.double().sum((0, 2, 3)).float(), (g.double() * xh.double()).sum((0, 2, 3)).float()
    invP = torch.tensor(1.0 / P, dtype=torch.float32)
    invPb = torch.tensor(1.0 / (P - 1), dtype=torch.float32) if dbeta_pm1 else invP
    inner = g - _ch(dbeta) * invPb - (0 if no_dgamma_term else xh * _ch(dgamma) * invP)
    out = {"dx": bf(_ch(i["gamma"] * istd) * inner), "dgamma": dgamma, "dbeta": dbeta}
    if c.res:
        out["dres"] = bf(g)
    return out


# ---------------------------------------------------------------------------------------------------------------- fusion sum
@functools.lru_cache(maxsize=None)
def fusion_inputs(c: FusionCase, seed: int = 0) -> dict:
    g = torch.Generator().manual_seed(3000 + 1000 * seed + FUSION_CASES.index(c) if c in FUSION_CASES else seed)
    return {"terms": [bf(torch.randn(c.B, c.C, c.H >> s, c.W >> s, generator=g)) for s in c.shifts],
            "dy": bf(torch.randn(c.B, c.C, c.H, c.W, generator=g))}


def nearest_up(t, s: int, offset: int = 0):
    """t[b, c, (y + offset) >> s, (x + offset) >> s] on the 2^s times larger grid (offset: a planted defect)"""
    if s == 0:
        return t
    H, W = t.shape[2] << s, t.shape[3] << s
    iy = ((torch.arange(H) + offset) >> s).clamp_max(t.shape[2] - 1)
    ix = ((torch.arange(W) + offset) >> s).clamp_max(t.shape[3] - 1)
    return t[:, :, iy][:, :, :, ix]


def block_sum(g, s: int):
    return g if s == 0 else F.avg_pool2d(g, 1 << s, divisor_override=1)


@functools.lru_cache(maxsize=None)
def fusion_forward_ref(c: FusionCase, seed: int = 0):
    terms = [t.double() for t in fusion_inputs(c, seed)["terms"]]
    ups = [nearest_up(t, s) for t, s in zip(terms, c.shifts)]
    ref = sum(ups)
    ref = F.relu(ref) if c.relu else ref
    return ref, U16 * ref.abs() + (len(terms) - 1) * U32 * sum(u.abs() for u in ups)


def fusion_backward_refs(c: FusionCase, out_kernel: torch.Tensor, seed: int = 0) -> list:
    """[(fp64 reference, allowed)] per term; the ReLU mask is out_kernel > 0"""
    g = fusion_inputs(c, seed)["dy"].double()
    if c.relu:
        g = g * (out_kernel.detach().cpu().double() > 0)
    refs = []
    for s in c.shifts:
        r = block_sum(g, s)
        refs.append((r, torch.zeros_like(r) if s == 0 else U16 * r.abs() + (4 ** s - 1) * U32 * block_sum(g.abs(), s)))
    return refs


def emulate_fusion(i: dict, c, offset: int = 0) -> torch.Tensor:
    v = i["terms"][0].clone()
    for t, s in zip(i["terms"][1:], c.shifts[1:]):
        v = v + nearest_up(t, s, offset)
    return bf(F.relu(v) if c.relu else v)


def emulate_fusion_backward(i: dict, c, out: torch.Tensor) -> list:
    g = i["dy"] * (out > 0) if c.relu else i["dy"]
    return [bf(block_sum(g, s)) for s in c.shifts]


if __name__ == "__main__":
    import sys
    import time
    torch.set_num_threads(16)
    t0 = time.time()
    res = measure_K(cases=[CONV_CASES[int(a)] for a in sys.argv[1:]] or None)
    for name, label in (("a", "(a) torch fp32 autograd"), ("b", "(b) sequential fp32")):
        top = max(res[name].items(), key=lambda kv: max(kv[1]))
        allmax = [max(v[s] for v in res[name].values()) for s in range(len(top[1]))]
        print(f"{label}: worst {max(top[1]):.3f} at {top[0]}; worst over the lattice per seed 0..5: " + " ".join(f"{v:.3f}" for v in allmax))
    print(f"{time.time() - t0:.0f} s")
