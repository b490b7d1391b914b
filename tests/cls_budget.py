"""fp64 references and per-element error budgets for the classifier's training tail: global average pool (forward / backward), the fp32
Linear (forward and its three gradients) and softmax cross-entropy with its gradient and hit counts (a plain module, like train_budget.py,
whose unit roundoffs and `check` it uses).

Every reference is fp64 on the CPU from the operands the kernel gets.  Every budget bounds what the kernel's number formats can lose,
from the unit roundoffs u16 (2^-8 for a bf16 store, 2^-11 for an fp16 store, plus ETA = 2^-25 below fp16's normal range, as in
train_budget_f16.py), u32 = 2^-24, u64 = 2^-53 and the same operation on absolute values; nothing in it is measured on the engine.

  pool forward (fp32)        A = (HW - 1) u32 mean|x| (a sum of HW addends in any order), allowed = A + u32 (|ref| + A) (the division)
  pool backward (16-bit)     allowed = u16 (|ref| + u32 |ref|) + u32 |ref| (+ ETA): one fp32 division, one store
  linear forward (fp32)      (K + 2) u32 (|x| |W|^T + |b|): K products and K additions in any order; dX: (N + 2) u32 |dY| |W|;
                             dW: (B + 2) u32 |dY|^T |x|; db: (B + 2) u32 sum|dY|
  cross-entropy              with d_j = z_j - max z (one fp32 subtraction: error u32 |d_j|) and e_j = expf(d_j), the relative error of e_j is
                             rho_j = u32 |d_j| + 2 EXPF_ULPS u32  (1 ulp <= 2^-23 = 2 u32 relative)
    loss (fp32)              the sum of the e_j and its logarithm are taken in double: a row's loss is off by at most sum_j p_j rho_j +
                             (N + 4) u64 (1 + |lse| + |z_t|); allowed = mean over the rows + u32 |loss| (the fp32 result)
    dlogits (fp32)           p_j = e_j * fl32(1 / sum): relative error rho_j + sum_k p_k rho_k + 2 u32; then p - onehot, times fl32(1 / B):
                             allowed = (p (rho_j + rho_bar + 2 u32) + u32 |p - onehot|) (1 + 2 u32) / B + 2 u32 |ref| + 2 TINY32
                             TINY32 = 2^-126: below it an fp32 result is subnormal or flushed (e_j for d_j < -87.3, and p_j / B)
    top-1 / top-5 hits, flag exact: integers from fp32 comparisons of the logits as given (rank rule of include/hhrnet.h)

EXPF_ULPS = 3: the OpenCL C specification's bound for exp on single precision (OpenCL C 3.0, section 7.4 "Relative error as ULPs": exp <= 3
ulp); the device's expf is ROCm's OCML exp_f32, the OpenCL math library, which is built to that table.  (The HIP math API page of the ROCm
documentation lists expf at 1 ulp; the looser, specified figure is used.)

The emulations are torch fp32 on the CPU with the kernels' operation order where the order is fixed (the pool's pixel-by-pixel sum, the
double sum of the e_j); test_cls_budget_cpu.py holds them inside every budget and shows that the planted defects leave it.
"""
from __future__ import annotations

import functools
from collections import namedtuple

import numpy as np
import torch

from train_budget import U32, U64, ConvCase, check  # noqa: F401  (check is re-exported for the tests)

U16 = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
ETA = {torch.bfloat16: 0.0, torch.float16: 2.0 ** -25}
EXPF_ULPS = 3      # see the docstring
TINY32 = 2.0 ** -126

PoolCase = namedtuple("PoolCase", "B HW C")
LinCase = namedtuple("LinCase", "B K N scale")  # scale: the logits are scaled so that max |z| is this (None: as they come)

POOL_CASES = [PoolCase(3, 49, 2048),   # the head at 224 x 224: a 7 x 7 map of 2048 channels
              PoolCase(2, 1, 2048),    # a 1 x 1 map (32 x 32 images): the mean of one pixel
              PoolCase(1, 4, 64)]      # one workgroup, mostly idle
LIN_CASES = [LinCase(1, 2048, 10, None),      # one row, N below one workgroup's four features
             LinCase(3, 2048, 1000, None),    # odd batch, fewer rows than the dX kernel's tile of 8
             LinCase(80, 2048, 1000, None),   # the reference's batch: every wave of the loss kernel takes five rows
             LinCase(5, 64, 1000, 80.0)]      # logits of +-80: exp(-160) underflows, exp(+80) without the max would be 5.5e34


# The classification head's conv shapes (224 x 224 images: maps of 56 .. 7; 32 x 32 images: 8 .. 1), which no case of
# train_budget.CONV_CASES reaches; they go through train_budget.conv_inputs / conv_refs / check as they stand.
HEAD_CONV_CASES = [
    ConvCase(256, 1024, 1, 1, 3, 7, 7, (0, 0)),     # chann_incr_blocks.3: conv3 and downsample
    ConvCase(1024, 2048, 1, 1, 3, 7, 7, (0, 0)),    # final_conv
    ConvCase(1024, 2048, 1, 1, 2, 1, 1, (0, 0)),    # final_conv on a 1 x 1 map
    ConvCase(256, 256, 3, 1, 3, 7, 7, (1, 1)),      # chann_incr_blocks.3.conv2
    ConvCase(256, 256, 3, 1, 2, 1, 1, (1, 1)),      # the same on a 1 x 1 map: eight of nine taps see padding only
    ConvCase(512, 1024, 3, 2, 3, 14, 14, (1, 1)),   # downsample_blocks.2
    ConvCase(512, 1024, 3, 2, 2, 2, 2, (1, 1)),     # the same, 2 x 2 -> 1 x 1
    ConvCase(128, 256, 3, 2, 3, 8, 8, (1, 1)),      # downsample_blocks.0 at 32 x 32 images
    ConvCase(128, 512, 1, 1, 3, 14, 14, (0, 0)),    # chann_incr_blocks.2: conv3
    ConvCase(32, 128, 1, 1, 3, 8, 8, (0, 0)),       # chann_incr_blocks.0: conv3 and downsample
]
# The weight gradient's sensitive bound (train_budget.K_SENSITIVE = 0.5 in units of sqrt(n) u32 S) was measured down to n = 48 pixels,
# the smallest sum of that lattice.  The three cases above that sum two pixels reach 0.707 of the unit from the reference side alone
# (the last rounding of a two-term sum, 1 / sqrt(2); torch fp32 autograd and sequential fp32 alike, seeds 0..2), every other case stays
# <= 0.33: below 48 pixels only the hard bound applies.
SENSITIVE_MIN_PIXELS = 48


def head_conv_pixels(c) -> int:
    return c.B * (c.H // c.stride) * (c.W // c.stride)


def pool_id(c) -> str:
    return f"{c.B}x{c.HW}x{c.C}"


def lin_id(c) -> str:
    return f"{c.B}x{c.K}x{c.N}" + (f"-pm{int(c.scale)}" if c.scale else "")


def rnd(t: torch.Tensor, dtype) -> torch.Tensor:
    return t.to(dtype).float()


# ---------------------------------------------------------------------------------------------------------------- pool
@functools.lru_cache(maxsize=None)
def pool_inputs(c: PoolCase, dtype=torch.bfloat16, seed: int = 0) -> dict:
    """x [B, HW, C] rounded to dtype (post-ReLU like: half of it zero), g fp32 [B, C]"""
    g = torch.Generator().manual_seed(4000 + 1000 * seed + POOL_CASES.index(c))
    return {"x": rnd(torch.randn(c.B, c.HW, c.C, generator=g).clamp_min(0) * 2, dtype), "g": torch.randn(c.B, c.C, generator=g)}


@functools.lru_cache(maxsize=None)
def pool_refs(c: PoolCase, dtype=torch.bfloat16, seed: int = 0) -> dict:
    """{fwd, bwd: (fp64 reference, allowed)}; bwd is [B, HW, C]"""
    i = pool_inputs(c, dtype, seed)
    x, g = i["x"].double(), i["g"].double()
    fwd = x.mean(1)
    A = (c.HW - 1) * U32 * x.abs().mean(1)
    bwd = (g / c.HW).unsqueeze(1).expand(c.B, c.HW, c.C).contiguous()
    a_b = U16[dtype] * (bwd.abs() * (1 + U32)) + U32 * bwd.abs() + ETA[dtype]
    return {"fwd": (fwd, A + U32 * (fwd.abs() + A)), "bwd": (bwd, a_b)}


def emulate_pool(i: dict, c: PoolCase, dtype=torch.bfloat16, count: int | None = None) -> dict:
    """the kernels' arithmetic: one fp32 accumulator over the pixels in order, an fp32 division.  count: a planted defect (the divisor)"""
    n = torch.tensor(float(c.HW if count is None else count), dtype=torch.float32)
    acc = torch.zeros(c.B, c.C)
    for p in range(c.HW):
        acc = acc + i["x"][:, p]
    return {"fwd": acc / n, "bwd": rnd((i["g"] / n).unsqueeze(1).expand(c.B, c.HW, c.C), dtype)}


# ---------------------------------------------------------------------------------------------------------------- linear
@functools.lru_cache(maxsize=None)
def lin_inputs(c: LinCase, seed: int = 0) -> dict:
    """fp32 x [B,K] (pooled ReLU outputs: non-negative), w [N,K], bias [N], dy [B,N]"""
    g = torch.Generator().manual_seed(5000 + 1000 * seed + LIN_CASES.index(c))
    x = torch.randn(c.B, c.K, generator=g).abs()
    w = torch.randn(c.N, c.K, generator=g) * c.K ** -0.5
    bias = torch.randn(c.N, generator=g) * 0.1
    if c.scale:
        k = c.scale / float((x.double() @ w.double().T + bias.double()).abs().max())
        w, bias = (w.double() * k).float(), (bias.double() * k).float()
    return {"x": x, "w": w, "bias": bias, "dy": torch.randn(c.B, c.N, generator=g) / c.B}


@functools.lru_cache(maxsize=None)
def lin_refs(c: LinCase, seed: int = 0) -> dict:
    """{fwd, dx, dw, db: (fp64 reference, allowed)}"""
    i = {k: v.double() for k, v in lin_inputs(c, seed).items()}
    a = {k: v.abs() for k, v in i.items()}
    return {"fwd": (i["x"] @ i["w"].T + i["bias"], (c.K + 2) * U32 * (a["x"] @ a["w"].T + a["bias"])),
            "dx": (i["dy"] @ i["w"], (c.N + 2) * U32 * (a["dy"] @ a["w"])),
            "dw": (i["dy"].T @ i["x"], (c.B + 2) * U32 * (a["dy"].T @ a["x"])),
            "db": (i["dy"].sum(0), (c.B + 2) * U32 * a["dy"].sum(0))}


def emulate_linear(i: dict, drop_last: bool = False) -> dict:
    """torch fp32.  drop_last: a planted defect, dW without the last sample of the batch"""
    n = i["x"].shape[0] - (1 if drop_last else 0)
    return {"fwd": i["x"] @ i["w"].T + i["bias"], "dx": i["dy"] @ i["w"], "dw": i["dy"][:n].T @ i["x"][:n], "db": i["dy"].sum(0)}


# ---------------------------------------------------------------------------------------------------------------- cross-entropy
def xent_targets(c: LinCase, seed: int = 0) -> torch.Tensor:
    """seeded targets in [0, N); the last row's is N - 1"""
    g = torch.Generator().manual_seed(6000 + 1000 * seed + LIN_CASES.index(c))
    t = torch.randint(0, c.N, (c.B,), generator=g)
    t[-1] = c.N - 1
    return t


def xent_logits(c: LinCase, seed: int = 0) -> torch.Tensor:
    """the fp32 logits of a linear case: its fp64 forward reference, rounded once"""
    return lin_refs(c, seed)["fwd"][0].float()


def tie_case():
    """-> (logits fp32 [6, 10], targets): exact ties around the target.  Ranks by the rule of include/hhrnet.h (ties to the lower index):
    row 0: three equal maxima, the target the last of them            -> rank 2: top-5 hit, top-1 miss
    row 1: the same, the target the first                             -> rank 0: both hit
    row 2: five logits above the target                               -> rank 5: both miss (a `<=` for `<` in hit-5 counts it)
    row 3: four above and one equal before the target                 -> rank 5: both miss
    row 4: four above and one equal AFTER the target                  -> rank 4: top-5 hit
    row 5: all ten equal, target 4                                    -> rank 4: top-5 hit"""
    z = torch.tensor([[1, 0, 2, 2, -1, 2, 0, 0, 0, 0],
                      [1, 0, 2, 2, -1, 2, 0, 0, 0, 0],
                      [5, 6, 7, 8, 9, 1, 0, 0, 0, 0],
                      [5, 6, 7, 8, 1, 1, 0, 0, 0, 0],
                      [5, 6, 7, 8, 1, 1, 0, 0, 0, 0],
                      [3, 3, 3, 3, 3, 3, 3, 3, 3, 3]], dtype=torch.float32) * 0.5
    return z, torch.tensor([5, 2, 5, 5, 4, 4]), (1, 4)  # expected (top-1 hits, top-5 hits)


def out_of_range_case():
    """-> (logits fp32 [4, 10], targets): rows 1 and 3 carry targets outside [0, N) (-1 and N)"""
    g = torch.Generator().manual_seed(77)
    return torch.randn(4, 10, generator=g), torch.tensor([3, -1, 9, 10])


def ranks(z: torch.Tensor, t: torch.Tensor, valid: torch.Tensor) -> torch.Tensor:
    """rank = #{j : z_j > z_t} + #{j < t : z_j == z_t} on the logits as given (no arithmetic: exact in any format)"""
    tc = t.clamp(0, z.shape[1] - 1)
    zt = z.gather(1, tc.view(-1, 1))
    j = torch.arange(z.shape[1]).view(1, -1)
    r = (z > zt).sum(1) + ((z == zt) & (j < tc.view(-1, 1))).sum(1)
    return torch.where(valid, r, torch.full_like(r, z.shape[1]))


def xent_refs(z: torch.Tensor, t: torch.Tensor) -> dict:
    """z fp32 [B,N], t int64 [B] -> {loss: (ref, allowed), dlogits: (ref, allowed), top1, top5, flags}"""
    B, N = z.shape
    valid = (t >= 0) & (t < N)
    tc = t.clamp(0, N - 1)
    zd = z.double()
    m = zd.max(1, keepdim=True).values
    d = zd - m
    lse = m + d.exp().sum(1, keepdim=True).log()
    p = (zd - lse).exp()
    zt = zd.gather(1, tc.view(-1, 1))
    v = valid.view(-1, 1).double()
    rows = (lse - zt) * v
    loss = rows.sum() / B
    rho = U32 * d.abs() + 2 * EXPF_ULPS * U32
    rho_bar = (p * rho).sum(1, keepdim=True)
    a_rows = (rho_bar + (N + 4) * U64 * (1 + lse.abs() + zt.abs())) * v
    a_loss = a_rows.sum() / B + U32 * loss.abs()
    oh = torch.zeros_like(zd).scatter_(1, tc.view(-1, 1), 1.0)
    ref = (p - oh) / B * v
    a_d = ((p * (rho + rho_bar + 2 * U32) + U32 * (p - oh).abs()) * (1 + 2 * U32) / B + 2 * U32 * ref.abs() + 2 * TINY32) * v
    r = ranks(z, t, valid)
    return {"loss": (loss.reshape(1), a_loss.reshape(1)), "dlogits": (ref, a_d), "top1": int((r < 1).sum()), "top5": int((r < 5).sum()),
            "flags": int((~valid).any())}


def emulate_xent(z: torch.Tensor, t: torch.Tensor, no_inv_b=False, no_max=False, le_for_lt=False, last_class_invalid=False) -> dict:
    """the kernel's arithmetic in torch fp32 (the sum of the exponentials and the logarithm in double); the flags are planted defects:
    the gradient without 1 / B, no max subtraction (plain fp32: exp, fp32 sum, fp32 log), hit-5 as rank <= 5, a target of N - 1 refused"""
    B, N = z.shape
    valid = (t >= 0) & (t < (N - 1 if last_class_invalid else N))
    tc = t.clamp(0, N - 1)
    v = valid.view(-1, 1)
    zt = z.gather(1, tc.view(-1, 1))
    if no_max:
        e = z.exp()
        s32 = e.sum(1, keepdim=True)
        rows = (s32.log() - zt).double()
        p = e / s32
    else:
        m = z.max(1, keepdim=True).values
        e = (z - m).exp()
        s = e.double().sum(1, keepdim=True)
        rows = (m.double() + s.log()) - zt.double()
        p = e * (1.0 / s).float()
    loss = ((rows * v).sum() / B).float()
    oh = torch.zeros_like(z).scatter_(1, tc.view(-1, 1), 1.0)
    dl = (p - oh) * (1.0 if no_inv_b else torch.tensor(1.0 / B, dtype=torch.float32)) * v
    r = ranks(z, t, valid)
    return {"loss": loss.reshape(1), "dlogits": dl, "top1": int((r < 1).sum()), "top5": int(((r <= 5) if le_for_lt else (r < 5)).sum()),
            "flags": int((~valid).any())}


def xent_mismatches(got: dict, refs: dict, what: str) -> list:
    """-> the names of the quantities of `got` that leave their budget or differ from the exact ones (empty: all inside)"""
    bad = []
    for k in ("loss", "dlogits"):
        try:
            check(got[k], *refs[k], f"{what} {k}", spatial=False)
        except AssertionError:
            bad.append(k)
    return bad + [k for k in ("top1", "top5", "flags") if got[k] != refs[k]]
