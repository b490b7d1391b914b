"""The reference of the heatmap panels (hh_heatmap_panels_u8, hh_unnormalize_u8, hh_resize_u8_scaled; keypoints/visualization.py
plot_heatmaps and the figure builders): the rule of include/hhrnet.h in numpy, whole maps at a time.

  maps       oracle.decode.bilinear, the C restatement of torch CPU's F.interpolate that tests/test_oracle_cpu.py pins to torch
             (test_bilinear_bit_exact_vs_torch_cpu); the stage average as results.py:225-226 forms it.
  pixels     the reference's own numpy expressions, quoted with file:line below.
  table      jet_lut's rule restated from its closed form 255 * clamp(1.5 - |4 i / 255 - c|, 0, 1), not from the integer form of the product.
  blend      render_ref.blend (addWeighted by the stated rule).
  grids      make_grid / np.concatenate / stack_horizontally of utils/image.py:15-61 written out.
  fx resize  a scale-parameterised copy of cv_resize.axis_taps / bilinear.

cv2 is not installed where the fixtures are made: the JET table and the fx / fy resize are UNPINNED against cv2 (include/hhrnet.h).
The keyword switches of `figure` / `resize_scaled` plant one defect each (tests/test_panels_cpu.py shows that the lattice tells every one
of them from the rule).  Shared by tests/test_panels_cpu.py, tests/test_gpu_panels.py and tools/panels_time.py."""
import numpy as np

import cv_resize
import render_ref as rr
from oracle import decode as orc

F = np.float32
DIRECT, SINGLE, NESTED, AVERAGE = 0, 1, 2, 3
CLIP, MINMAX = 1, 2
MEAN = np.array([0.485, 0.456, 0.406])  # base/transforms/base.py:5-6
STD = np.array([0.229, 0.224, 0.225])


def jet_lut():
    """uint8 [256,3] in B,G,R order: round(255 * clamp(1.5 - |4 i / 255 - c|, 0, 1)) for c = 1 (B), 2 (G), 3 (R), in exact rational
    arithmetic: 255 * (1.5 - |4i/255 - c|) = (765 - |8i - 510c|) / 2, halves rounded up."""
    from fractions import Fraction
    out = np.zeros((256, 3), np.uint8)
    for i in range(256):
        for ch, c in enumerate((1, 2, 3)):
            v = 255 * min(max(Fraction(3, 2) - abs(Fraction(4 * i, 255) - c), 0), 1)
            out[i, ch] = int(v + Fraction(1, 2))  # floor(v + 1/2)
    return out


def quantise(hm):
    """visualization.py:105-106: hm = (hm * 255).astype(np.uint8); hm = 255 - hm."""
    with np.errstate(invalid="ignore", over="ignore"):
        hm = (hm * 255).astype(np.uint8)
    return 255 - hm


def map_values(kind, src, src2, H, W, *, nested_as_single=False):
    """One map's full-resolution values fp32 [H,W]."""
    src = np.ascontiguousarray(src, F)
    if kind == DIRECT:
        assert src.shape == (H, W)
        return src
    if kind == SINGLE or (kind == NESTED and nested_as_single):
        return orc.bilinear(src[None], H, W)[0]                      # results.py:64-67 resize_heatmaps
    h, w = src.shape
    assert (4 * h, 4 * w) == (H, W)
    half = orc.bilinear(src[None], 2 * h, 2 * w)[0]                  # results.py:48-54 match_heatmaps_size
    if kind == AVERAGE:
        with np.errstate(invalid="ignore", over="ignore"):
            half = (half + np.ascontiguousarray(src2, F)) / F(2)     # results.py:226 torch.stack(...).mean(dim=0) of two stages
    return orc.bilinear(half[None], H, W)[0]


def cell(image, hm, flags, lut, *, minus_min=False, drop_nan=False, half_up=False, swap_lut=False):
    """visualization.py:100-109 on one map fp32 [H,W] -> uint8 [H,W,3]."""
    hm = hm.astype(F)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        if flags & CLIP:
            hm = np.clip(hm, 0, 1)                                   # :102
        if flags & MINMAX:
            mx, mn = (np.nanmax(hm), np.nanmin(hm)) if drop_nan else (hm.max(), hm.min())
            hm = (hm - (mn if minus_min else mx)) / (mx - mn)        # :104  (hm - hm.max()) / (hm.max() - hm.min())
        assert hm.dtype == F
        idx = quantise(hm)                                           # :105-106
    colour = (lut[:, ::-1] if swap_lut else lut)[idx]                # :107 applyColorMap, channel for channel
    if half_up:
        v = np.floor(image.astype(F) * F(0.25) + colour.astype(F) * F(0.75) + F(0.5))
        return np.clip(v, 0, 255).astype(np.uint8)
    return rr.blend(image, colour, 0.75)                             # :108 addWeighted(image, 0.25, hm, 0.75, 0)


def grid_layout(n, nrows, H, W, pad):
    """utils/image.py:25-36 -> (grid_h, grid_w, [(y, x) of every cell])."""
    ncols = int(np.ceil(n / nrows).item())
    return (H + pad) * nrows + pad, (W + pad) * ncols + pad, [(pad + (i // ncols) * (H + pad), pad + (i % ncols) * (W + pad)) for i in range(n)]


def make_grid(images, nrows=1, pad=5, *, stale_last=False):
    """utils/image.py:15-38.  `stale_last`: the cells that stay unused are left as 0xA5 instead of zero."""
    H, W = images[0].shape[:2]
    gh, gw, at = grid_layout(len(images), nrows, H, W, pad)
    grid = np.zeros((gh, gw, 3), np.uint8)
    if stale_last:
        ncols = (gw - pad) // (W + pad)
        for i in range(len(images), nrows * ncols):
            y, x = pad + (i // ncols) * (H + pad), pad + (i % ncols) * (W + pad)
            grid[y:y + H, x:x + W] = 0xA5
    for (y, x), im in zip(at, images):
        grid[y:y + H, x:x + W] = im
    return grid


def figure(image, grids, lut, **defect):
    """The grids of a figure stacked vertically (np.concatenate(..., axis=0): results.py:152, :327).  grids: list of
    (maps, nrows, pad), maps a list of (kind, src, src2, flags)."""
    grid_defect = {k: defect.pop(k) for k in ("stale_last",) if k in defect}
    value_defect = {k: defect.pop(k) for k in ("nested_as_single",) if k in defect}
    H, W = image.shape[:2]
    out = []
    for maps, nrows, pad in grids:
        cells = [cell(image, map_values(kind, src, src2, H, W, **value_defect), flags, lut, **defect) for kind, src, src2, flags in maps]
        out.append(make_grid(cells, nrows, pad, **grid_defect))
    return np.concatenate(out, axis=0)


def inverse_transform(x):
    """base/transforms/base.py:38-41 on a float32 [3,H,W] array."""
    image_npy = np.asarray(x, F).transpose(1, 2, 0)
    image_npy = (image_npy * STD) + MEAN
    with np.errstate(invalid="ignore", over="ignore"):
        return (image_npy * 255).astype(np.uint8)


def scaled_size(n, f):
    """cvRound(n * f): to nearest, half to even."""
    return int(np.rint(np.float64(n) * np.float64(f)))


def _axis_taps(dst, src, scale, column):
    """cv_resize.axis_taps with the scale given."""
    d = np.arange(dst, dtype=np.float64)
    f = ((d + 0.5) * scale - 0.5).astype(F)
    s = np.floor(f).astype(np.int32)
    f = f - s.astype(F)
    if column:
        low, high = s < 0, s >= src - 1
        s = np.where(low, 0, np.where(high, src - 1, s)).astype(np.int32)
        f = np.where(low | high, F(0), f).astype(F)
        i0, i1 = s, np.minimum(s + 1, src - 1)
    else:
        i0, i1 = np.clip(s, 0, src - 1), np.clip(s + 1, 0, src - 1)
    w0 = np.rint((F(1) - f) * F(cv_resize.COEF_ONE)).astype(np.int16).astype(np.int32)
    w1 = np.rint(f * F(cv_resize.COEF_ONE)).astype(np.int16).astype(np.int32)
    return i0.astype(np.int32), i1.astype(np.int32), w0, w1


def resize_scaled(src, fx, fy, *, size_ratio=False):
    """cv2.resize(src, (0, 0), fx=fx, fy=fy) for a uint8 [h,w,c] array: dsize = (cvRound(w fx), cvRound(h fy)), scale = 1 / f.
    `size_ratio`: the scales of cv2.resize(src, dsize) instead (1 / (W / w))."""
    src = np.ascontiguousarray(src)
    assert src.dtype == np.uint8 and src.ndim == 3
    h, w = src.shape[:2]
    H, W = scaled_size(h, fy), scaled_size(w, fx)
    s = src.astype(np.int32)
    if h == 2 * H and w == 2 * W:
        out = cv_resize.area_2x2(s)
    else:
        sx, sy = (1.0 / (float(W) / w), 1.0 / (float(H) / h)) if size_ratio else (1.0 / float(fx), 1.0 / float(fy))
        x0, x1, a0, a1 = _axis_taps(W, w, sx, True)
        y0, y1, b0, b1 = _axis_taps(H, h, sy, False)
        hor = s[:, x0] * a0[None, :, None] + s[:, x1] * a1[None, :, None]
        h0, h1 = hor[y0], hor[y1]
        out = (((b0[:, None, None] * (h0 >> 4)) >> 16) + ((b1[:, None, None] * (h1 >> 4)) >> 16) + 2) >> 2
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def stack_horizontally(images, pad=5):
    """utils/image.py:41-61 with cv_resize.resize for cv2.resize."""
    new_h = max(im.shape[0] for im in images)
    resized = []
    for im in images:
        h, w = im.shape[:2]
        resized.append(im if h == new_h else cv_resize.resize(im, (int(w / h * new_h), new_h)))
    grid = np.zeros((pad + new_h + pad, sum(im.shape[1] + pad for im in resized) + pad, 3), np.uint8)
    x = pad
    for im in resized:
        grid[pad:-pad, x:x + im.shape[1]] = im
        x += im.shape[1] + pad
    return grid


def inference_figure(image, hm_q, hm_h, tags_q, lut, **defect):
    """InferenceKeypointsResult.plot()["heatmaps"] (results.py:317-328) from the stage outputs [K,h,w] / [K,2h,2w] / [K,h,w]."""
    grids = [([(AVERAGE, q, h, MINMAX) for q, h in zip(hm_q, hm_h)], 2, 5), ([(SINGLE, t, None, MINMAX) for t in tags_q], 2, 5)]
    resize_defect = {k: defect.pop(k) for k in ("size_ratio",) if k in defect}
    return resize_scaled(figure(image, grids, lut, **defect), 0.6, 0.6, **resize_defect)


def validation_figure(image, connections, hm_q, hm_h, tags_q, lut, **defect):
    """KeypointsResult.plot()["heatmaps"] (results.py:126-155): `connections` is the overlay on `image`."""
    grids = [([(NESTED, q, None, CLIP) for q in hm_q], 1, 5), ([(SINGLE, t, None, MINMAX) for t in tags_q], 1, 5),
             ([(SINGLE, h, None, CLIP) for h in hm_h], 1, 5)]
    resize_defect = {k: defect.pop(k) for k in ("size_ratio",) if k in defect}
    return stack_horizontally([connections, resize_scaled(figure(image, grids, lut, **defect), 0.4, 0.4, **resize_defect)])
