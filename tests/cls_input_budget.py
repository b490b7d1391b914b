"""Reference, case lattice and per-element error budget of the classifier's device-built input (hh_resized_crop_u8_batch,
classification/input.py).  A plain module, like train_budget.py; nothing in it is measured on the kernel.

Reference.  `restate` is the semantics of include/hhrnet.h in numpy float64: crop -> ToTensor -> separable triangle-filter resample
(horizontal, then vertical) -> window -> flip -> normalise.  `torch_cpu` is the pipeline the kernel replaces, on torch's own fp32 CPU
kernels: F.interpolate(mode="bilinear", antialias=...) on the cropped ToTensor image, the window, the flip, sub / div.

Budget (first order in u = 2^-24; `budget` returns it per element, [3,H,W]).  Per axis and output index i, with n = taps + 2 (a tap at
the edge of the support has weight ~0 and may be in or out of the fp32 range), T = the float64 sum of the raw weights:
  position    the centre scale (i + 0.5) is formed at magnitudes up to the crop extent: fl(in / out) and the product give 2 u centre;
              (j - centre) and + 0.5 are two roundings of a number below support + 1: d_pos = 2 u (centre + support + 1)
  raw weight  the position scaled by 1 / support (rounded reciprocal, rounded product) and 1 - |t|: e_raw = d_pos / support + 3 u
              -- this is the term that grows like ulp32(extent) / support
  normalised  w = raw / sum(raw): sum_j |dw_j| <= E_w = 2 n e_raw / T + (n + 1) u   (the raw errors, the sum's own error, the division)
  one pass    sum_j w_j v_j with 0 <= v <= 1 in fp32, products and sums rounded separately, any order: E_w + (n + 1) u
The horizontal pass carries ToTensor's u (v = fl(b / 255) <= 1); the vertical pass' weights sum to 1, so it passes the horizontal
error of the column through and adds its own.  In [0,1] units: e01[y,x] = u + pass_x[x] + pass_y[y].  Normalise is one fp32
subtraction and one fp32 division: allowed[c,y,x] = e01[y,x] / std_c + 3 u |ref[c,y,x]|.
Every term is a worst case over signs (an L1 bound), so it is not tight: for 375x500 -> 224^2 it allows 1.7e-4 in [0,1] units where
torch's fp32 result differs from float64 by 1.3e-5 (measured, for orientation only).  It still sits three orders of magnitude below
what a misplaced tap does on the noise images of the lattice (test_cls_input_cpu.py asserts a factor of 100 for every seeded mistake).
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

U32 = 2.0 ** -24
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)

# one sample: raw image h x w (seeded noise), source rectangle, virtual size, window origin, output H x W, flip, antialias
Case = namedtuple("Case", "name h w top left ch cw rh rw oy ox H W flip aa seed")


def _whole(name, h, w, S, flip, aa, seed):
    return Case(name, h, w, 0, 0, h, w, S, S, 0, 0, S, S, flip, aa, seed)


def _crop(name, h, w, rect, S, flip, aa, seed):
    return Case(name, h, w, *rect, S, S, 0, 0, S, S, flip, aa, seed)


CASES = [
    # ---- 16 x 16
    _whole("down-37x53", 37, 53, 16, 0, 1, 1),                     # scale 2.3 / 3.3: 5..8 taps an axis
    _whole("down-37x53-flip", 37, 53, 16, 1, 1, 1),
    _whole("down-37x53-noaa", 37, 53, 16, 0, 0, 1),                # the same without the antialias: 2 taps
    _whole("up-13x9-flip", 13, 9, 16, 1, 1, 2),                    # scale < 1: support 1
    _whole("up-13x9-noaa", 13, 9, 16, 0, 0, 2),
    Case("window-120x47", 120, 47, 0, 0, 120, 47, 16, 24, 0, 5, 16, 16, 0, 1, 3),       # 16 x 24 virtual, window at (0, 5): asymmetric
    Case("window-120x47-flip", 120, 47, 0, 0, 120, 47, 16, 24, 0, 5, 16, 16, 1, 1, 3),
    Case("window-120x47-noaa", 120, 47, 0, 0, 120, 47, 16, 24, 0, 5, 16, 16, 1, 0, 3),
    _crop("one-pixel", 21, 30, (9, 17, 1, 1), 16, 0, 1, 4),        # a 1 x 1 crop: every output is that pixel
    _crop("corner-tl", 37, 53, (0, 0, 20, 25), 16, 0, 1, 5),       # a crop in each image corner: the clamp is at the crop, the image goes on
    _crop("corner-tr", 37, 53, (0, 28, 20, 25), 16, 1, 1, 5),
    _crop("corner-bl", 37, 53, (17, 0, 20, 25), 16, 0, 0, 5),
    _crop("corner-br", 37, 53, (17, 28, 20, 25), 16, 1, 1, 5),
    _crop("inner-crop", 64, 80, (11, 13, 40, 50), 16, 0, 1, 6),    # pixels of the image on every side of the crop
    _whole("identity-whole", 16, 16, 16, 0, 1, 7),                 # extent == virtual size: bit-identical
    _crop("identity-inner-flip", 37, 53, (3, 5, 16, 16), 16, 1, 1, 7),
    _crop("identity-inner-noaa", 37, 53, (21, 37, 16, 16), 16, 0, 0, 7),
    # ---- 8 x 8
    _whole("tall-500x40", 500, 40, 8, 0, 1, 8),                    # scale 62.5: 126 vertical taps, several LDS chunks
    _whole("tall-500x40-flip-noaa", 500, 40, 8, 1, 0, 8),
    _crop("down-8-crop", 37, 53, (5, 7, 30, 41), 8, 1, 1, 9),
    # ---- the inference form: Resize 32 + CenterCrop 28 / 29 of 40 x 70 (29: odd width, and offsets where round and floor differ)
    Case("infer-40x70-28", 40, 70, 0, 0, 40, 70, 32, 56, 2, 14, 28, 28, 0, 1, 10),
    Case("infer-40x70-28-noaa", 40, 70, 0, 0, 40, 70, 32, 56, 2, 14, 28, 28, 0, 0, 10),
    _crop("crop-28-flip", 64, 80, (11, 13, 40, 50), 28, 1, 1, 6),   # (a second raw size in the 28 x 28 batch)
    Case("infer-40x70-29", 40, 70, 0, 0, 40, 70, 32, 56, 2, 14, 29, 29, 0, 1, 10),
    Case("window-odd-flip", 50, 60, 0, 0, 50, 60, 29, 40, 0, 4, 29, 29, 1, 1, 11),      # odd width, asymmetric window (4 left, 7 right)
    _crop("crop-odd-flip", 33, 41, (2, 3, 30, 35), 29, 1, 1, 12),
    _crop("crop-odd", 33, 41, (2, 3, 30, 35), 29, 0, 1, 12),
]
IDENTITY = [c.name for c in CASES if (c.ch, c.cw) == (c.rh, c.rw)]
assert len({c.name for c in CASES}) == len(CASES) and len(IDENTITY) == 3


def image_of(case: Case) -> np.ndarray:
    """The case's raw image: seeded uint8 noise (neighbouring pixels unrelated: a misplaced tap shows)."""
    return np.random.RandomState(1000 + case.seed).randint(0, 256, (case.h, case.w, 3)).astype(np.uint8)


def axis_taps(in_: int, out: int, antialias: bool, lo_limit: int = 0, hi_limit: int | None = None):
    """Per output index: (first tap, raw float64 weights, support, centre).  Taps are clamped to [lo_limit, hi_limit): [0, in) in
    the semantics; the seeded mistake 'clamp_image' passes the image's range instead."""
    hi_limit = in_ if hi_limit is None else hi_limit
    scale = in_ / out
    support = max(scale, 1.0) if antialias else 1.0
    taps = []
    for i in range(out):
        centre = scale * (i + 0.5)
        lo, hi = max(lo_limit, int(centre - support + 0.5)), min(hi_limit, int(centre + support + 0.5))
        j = np.arange(lo, hi)
        raw = np.maximum(0.0, 1.0 - np.abs((j - centre + 0.5) / support))
        taps.append((lo, raw, support, centre))
    return taps


def axis_matrix(in_: int, out: int, antialias: bool, dtype=np.float64, lo_limit: int = 0, hi_limit: int | None = None, offset: int = 0, width=None):
    """[out, width] matrix of normalised weights over source positions `offset + tap`."""
    m = np.zeros((out, in_ if width is None else width), dtype)
    for i, (lo, raw, _, _) in enumerate(axis_taps(in_, out, antialias, lo_limit, hi_limit)):
        m[i, offset + lo:offset + lo + len(raw)] = (raw / raw.sum()).astype(dtype)
    return m


def restate(img: np.ndarray, c: Case, mean=MEAN, std=STD, dtype=np.float64, mistake: str | None = None) -> np.ndarray:
    """The semantics of hh_resized_crop_u8_batch for one sample -> [3,H,W] of `dtype` (float32: the same operations in fp32, for the
    identity crops, where every weight is exactly 1 or 0).  `mistake` seeds one of the defects the budget has to catch."""
    aa = bool(c.aa) and mistake != "no_antialias"
    ox = c.ox + (1 if mistake == "origin_off_by_one" else 0)
    x = img.astype(dtype) / dtype(255)                                   # ToTensor, [h,w,3]
    if mistake == "clamp_image":  # taps leave the crop and read the image around it
        my = axis_matrix(c.ch, c.rh, aa, dtype, -c.top, c.h - c.top, c.top, c.h)
        mx = axis_matrix(c.cw, c.rw, aa, dtype, -c.left, c.w - c.left, c.left, c.w)
        src = x
    else:
        my, mx = axis_matrix(c.ch, c.rh, aa, dtype), axis_matrix(c.cw, c.rw, aa, dtype)
        src = x[c.top:c.top + c.ch, c.left:c.left + c.cw]
        if mistake == "flip_source" and c.flip:
            src = src[:, ::-1]
    hpass = np.einsum("xj,rjc->rxc", mx, src)                            # horizontal first
    v = np.einsum("yr,rxc->cyx", my, hpass)                              # [3,rh,rw]
    win = v[:, c.oy:c.oy + c.H, ox:ox + c.W]
    if c.flip and mistake != "flip_source":
        win = win[:, :, ::-1]
    m, s = np.asarray(mean, np.float32).astype(dtype), np.asarray(std, np.float32).astype(dtype)
    return (win - m[:, None, None]) / s[:, None, None]


def torch_cpu(img: np.ndarray, c: Case, mean=MEAN, std=STD) -> torch.Tensor:
    """What the kernel replaces, on torch's fp32 CPU kernels -> [3,H,W] fp32."""
    x = torch.from_numpy(img).permute(2, 0, 1).float().div(255)          # ToTensor
    x = x[:, c.top:c.top + c.ch, c.left:c.left + c.cw]
    v = F.interpolate(x[None], size=(c.rh, c.rw), mode="bilinear", align_corners=False, antialias=bool(c.aa))[0]
    win = v[:, c.oy:c.oy + c.H, c.ox:c.ox + c.W]
    if c.flip:
        win = win.flip(-1)
    m, s = torch.tensor(mean, dtype=torch.float32), torch.tensor(std, dtype=torch.float32)
    return win.sub(m[:, None, None]).div(s[:, None, None]).contiguous()


def _pass_error(in_: int, out: int, antialias: bool) -> np.ndarray:
    """[out]: the error of one fp32 pass over values in [0, 1] (see the module docstring)."""
    err = np.zeros(out)
    for i, (_, raw, support, centre) in enumerate(axis_taps(in_, out, antialias)):
        n, T = len(raw) + 2, raw.sum()
        d_pos = 2 * U32 * (centre + support + 1)
        e_raw = d_pos / support + 3 * U32
        e_w = 2 * n * e_raw / T + (n + 1) * U32
        err[i] = e_w + (n + 1) * U32
    return err


def budget(c: Case, ref: np.ndarray, std=STD) -> np.ndarray:
    """Allowed |result - ref| per element, [3,H,W], for the float64 reference `ref` of the case."""
    ex, ey = _pass_error(c.cw, c.rw, bool(c.aa)), _pass_error(c.ch, c.rh, bool(c.aa))
    ex = ex[c.ox:c.ox + c.W]
    if c.flip:
        ex = ex[::-1]
    e01 = U32 + ex[None, :] + ey[c.oy:c.oy + c.H, None]
    s = np.asarray(std, np.float32).astype(np.float64)
    return e01[None] / s[:, None, None] + 3 * U32 * np.abs(ref)


def worst_ratio(got, ref: np.ndarray, allowed: np.ndarray) -> float:
    """max over ALL elements of |got - ref| / allowed (nothing is left out; a NaN counts as infinite)."""
    got = np.asarray(got, np.float64)
    assert got.shape == ref.shape == allowed.shape, (got.shape, ref.shape, allowed.shape)
    r = np.abs(got - ref) / allowed
    return float("inf") if not np.isfinite(r).all() else float(r.max())
