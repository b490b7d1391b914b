"""Pose overlays: `plot_connections` of the reference (keypoints/visualization.py:13-90) with the per-pixel work on the GPU.

The host does the small float64 / integer bookkeeping (`build_primitives`: which primitives, in what order, where, how large, which
colour), one hh_render_poses_u8_batch launch draws and blends a batch of frames.  The drawing rule, its rasterisation and the stated
deviation from OpenCV's rasteriser are written at hh_render_poses_u8_batch in include/hhrnet.h.  There is no CPU fallback.

Heatmap panels: `plot_heatmaps`, `make_grid`, `np.concatenate` and `stack_horizontally` of the reference (visualization.py:93-110,
utils/image.py:15-61).  The host does the integer bookkeeping (`figure_layout`: cell origins, canvas size); hh_heatmap_panels_u8
resamples, colours, blends and tiles every map of a figure in one call from the stage outputs as they are, hh_resize_u8_scaled shrinks
the figure, and only the finished uint8 figure crosses to the host.  The per-pixel rule and what is UNPINNED for want of cv2 (the JET
table, the fx / fy resize) are written at hh_heatmap_panels_u8 in include/hhrnet.h.
"""
from __future__ import annotations

import numpy as np
import torch

from .. import _lib
from .._stage import Block, Layout, fill_frames, frames_to_host, per_frame, place_frames

PRIM, DESC = _lib.struct_dtype("hh_render_prim"), _lib.struct_dtype("hh_render_desc")
DISC, RING, ELLIPSE = (_lib.const(k) for k in ("RENDER_DISC", "RENDER_RING", "RENDER_ELLIPSE"))
MAX_PRIMS = _lib.const("RENDER_MAX_PRIMS")
MAX_SIDE = 16384
MAX_COORD = 1 << 23
FLAG_BGR = 1

# utils/image.py:168-195 (`colors`, get_color): 20 entries repeated five times; tests/golden/render.npz records get_color(0..99)
_COLORS = [(144, 238, 144), (255, 105, 180), (135, 206, 250), (255, 215, 0), (255, 69, 0), (255, 182, 193), (0, 128, 128), (255, 160, 122),
           (0, 191, 255), (70, 130, 180), (255, 99, 71), (0, 255, 255), (0, 255, 127), (255, 0, 255), (255, 215, 0), (255, 140, 0),
           (30, 144, 255), (255, 20, 147), (255, 165, 0), (218, 112, 214)]
DEFAULT_PALETTE = np.array(_COLORS * 5, dtype=np.uint8)


def blend_weights(alpha: float) -> tuple[np.float32, np.float32]:
    """addWeighted(image, 1 - alpha, connections_image, alpha, 0): both weights formed in double, rounded once to fp32."""
    alpha = float(alpha)
    if not np.isfinite(alpha):
        raise ValueError("alpha must be finite")
    return np.float32(1.0 - alpha), np.float32(alpha)


def _box(cx: int, cy: int, ex: int, ey: int):
    """Inclusive box centre +- extent clipped to 0..16383; wholly outside -> empty (x1 < x0 or y1 < y0)."""
    return (min(max(cx - ex, 0), MAX_SIDE), min(max(cy - ey, 0), MAX_SIDE), min(max(cx + ex, -1), MAX_SIDE - 1), min(max(cy + ey, -1), MAX_SIDE - 1))


def _boxes(cx, cy, ex, ey) -> np.ndarray:
    """_box on arrays -> [..., 4]."""
    return np.clip(cx - ex, 0, MAX_SIDE), np.clip(cy - ey, 0, MAX_SIDE), np.clip(cx + ex, -1, MAX_SIDE - 1), np.clip(cy + ey, -1, MAX_SIDE - 1)


def ellipse_prim(cx: int, cy: int, a: int, b: int, c, s, colour) -> tuple:
    """One hh_render_prim row: the filled ellipse with semi-axes a + 1/2 along (c, s) and b + 1/2 across, c and s rounded to fp32 here."""
    if a > 32767 or b > 32767:
        raise ValueError("ellipse axis beyond 32767 pixels")
    c, s = np.float32(c), np.float32(s)
    # half extents of the rotated ellipse plus 2: beyond the fp32 rounding of the inside test
    ha, hb, cd, sd = a + 0.5, b + 0.5, float(c), float(s)
    ex, ey = int(np.sqrt((ha * cd) ** 2 + (hb * sd) ** 2)) + 2, int(np.sqrt((ha * sd) ** 2 + (hb * cd) ** 2)) + 2
    return (cx, cy, 2 * a + 1, 2 * b + 1, c, s, tuple(colour)[:3], ELLIPSE, *_box(cx, cy, ex, ey))


def circle_prim(cx: int, cy: int, radius: int, colour, ring: bool = False) -> tuple:
    """One hh_render_prim row: the filled disc of `radius`, or the one-pixel ring of `radius` (ring=True)."""
    if not 1 <= radius <= 32767:
        raise ValueError("radius outside 1..32767")
    return (cx, cy, radius, radius, 1.0, 0.0, tuple(colour)[:3], RING if ring else DISC, *_box(cx, cy, radius, radius))


def table_of(rows: list) -> np.ndarray:
    table = np.zeros(len(rows), PRIM)
    for n, row in enumerate(rows):
        table[n] = row
    return table


def build_primitives(coords, scores, limbs, thr, color_mode, palette=DEFAULT_PALETTE, alpha: float = 0.8, return_direction: bool = False, ids=None):
    """The primitive table of one frame in draw order (structured array of hh_render_prim): numpy only, float64 / int64.
    coords [P,K,2] (x, y), scores [P,K] or [P,K,1]; `limbs` may be None (keypoints only).  `alpha` is only checked (the weights
    belong to the frame's descriptor: blend_weights).  Raises where the reference would raise (a palette shorter than needed) and
    where the table cannot express the frame (a coordinate beyond +-2^23, an axis or radius beyond 32767).
    `return_direction`: also the float64 (c, s) of every row before its one rounding to fp32 ([N,2]; (1, 0) for discs and rings).
    color_mode "track" (an extension, keypoints/tracking.py): `ids` [P] are the people's track ids; a person is drawn like in "person"
    mode but in palette row (id - 1) % len(palette), whatever its row, and a person with id 0 is not drawn."""
    blend_weights(alpha)
    if color_mode not in ("person", "limb", "track"):
        raise ValueError(f"color_mode {color_mode!r} is not 'person', 'limb' or 'track'")
    coords = np.asarray(coords, dtype=np.float64)
    if color_mode == "track":
        if ids is None:
            raise ValueError("color_mode 'track' needs ids")
        ids = np.asarray(ids, dtype=np.int64).reshape(-1)
        if len(ids) != len(coords):
            raise ValueError(f"{len(ids)} ids for {len(coords)} people")
        tracked = ids != 0
        coords, scores, ids = coords[tracked], np.asarray(scores, dtype=np.float64).reshape(len(ids), -1)[tracked], ids[tracked]
    P = len(coords)
    if P == 0:
        return (np.zeros(0, PRIM), np.zeros((0, 2))) if return_direction else np.zeros(0, PRIM)
    scores = np.asarray(scores, dtype=np.float64).reshape(P, -1)
    K = coords.shape[1]
    assert coords.shape == (P, K, 2) and scores.shape == (P, K)
    if not np.isfinite(coords).all():
        raise ValueError("non-finite keypoint coordinate")
    palette = np.asarray(palette)
    limbs = list(limbs) if limbs is not None else []
    need = P if color_mode == "person" else 1 if color_mode == "track" else max(len(limbs), K)
    if len(palette) < need:
        raise IndexError(f"palette of {len(palette)} colours, {need} needed")
    xy = np.trunc(coords)  # int(): toward zero
    if np.abs(xy).max() > MAX_COORD:
        raise ValueError("keypoint coordinate beyond +-2^23")
    xy = xy.astype(np.int64)
    size = np.maximum(2, ((coords[..., 1].max(1) - coords[..., 1].min(1)) / 100).astype(np.int32)).astype(np.int64)  # over ALL K keypoints
    if size.max() + 1 > 32767:
        raise ValueError("draw size beyond 32766")
    drawn = ~(scores < float(thr))  # a score equal to thr is drawn
    L = len(limbs)
    # every possible row of every person, [P, L + 2K]: the limbs, then disc and ring of each keypoint; the rows that are drawn are
    # picked at the end, which keeps this order
    full = np.zeros((P, L + 2 * K), PRIM)
    dirs = np.zeros((P, L + 2 * K, 2))
    dirs[..., 0] = 1.0
    keep = np.zeros((P, L + 2 * K), bool)
    person = np.arange(P)[:, None] if color_mode != "track" else ((ids - 1) % len(palette))[:, None]
    if L:
        k0, k1 = np.array(limbs, np.int64).reshape(L, 2).T
        x1, y1, x2, y2 = xy[:, k0, 0], xy[:, k0, 1], xy[:, k1, 0], xy[:, k1, 1]
        dx, dy = x2 - x1, y2 - y1
        hyp = np.sqrt((dx * dx + dy * dy).astype(np.float64))
        half = hyp.astype(np.int64) // 2
        major = np.abs(dx) > np.abs(dy)
        safe = np.where(hyp == 0, 1.0, hyp)
        c = np.where(hyp == 0, 1.0, np.where(major, dx, dy) / safe)
        s = np.where(hyp == 0, 0.0, np.where(major, dy, -dx) / safe)
        a, b = np.where(major, half, size[:, None]), np.where(major, size[:, None], half)
        valid = drawn[:, k0] & drawn[:, k1]
        if (valid & (half > 32767)).any():
            raise ValueError("limb longer than 65535 pixels")
        a, b = np.minimum(a, 32767), np.minimum(b, 32767)  # (rows that are not drawn)
        c32, s32 = c.astype(np.float32), s.astype(np.float32)
        # half extents of the rotated ellipse with semi-axes a + 1/2, b + 1/2, plus 2: beyond the fp32 rounding of the inside test
        ha, hb, cd, sd = a + 0.5, b + 0.5, c32.astype(np.float64), s32.astype(np.float64)
        ex = np.sqrt((ha * cd) ** 2 + (hb * sd) ** 2).astype(np.int64) + 2
        ey = np.sqrt((ha * sd) ** 2 + (hb * cd) ** 2).astype(np.int64) + 2
        cx, cy = (x1 + x2) // 2, (y1 + y2) // 2  # floor division
        e = full[:, :L]
        e["cx"], e["cy"], e["A"], e["B"], e["c"], e["s"], e["kind"] = cx, cy, 2 * a + 1, 2 * b + 1, c32, s32, ELLIPSE
        e["rgb"] = palette[person if color_mode != "limb" else np.arange(L)[None, :], :3] + np.zeros((P, L, 1), np.uint8)
        e["x0"], e["y0"], e["x1"], e["y1"] = _boxes(cx, cy, ex, ey)
        dirs[:, :L, 0], dirs[:, :L, 1] = c, s
        keep[:, :L] = valid
    for ring in (0, 1):
        k = full[:, L + ring::2]
        radius = (size + ring)[:, None] + np.zeros((P, K), np.int64)
        k["cx"], k["cy"], k["A"], k["B"], k["c"], k["kind"] = xy[..., 0], xy[..., 1], radius, radius, 1.0, RING if ring else DISC
        if not ring:
            k["rgb"] = palette[person if color_mode != "limb" else np.arange(K)[None, :], :3] + np.zeros((P, K, 1), np.uint8)
        k["x0"], k["y0"], k["x1"], k["y1"] = _boxes(xy[..., 0], xy[..., 1], radius, radius)
        keep[:, L + ring::2] = drawn
    table = np.ascontiguousarray(full[keep])
    return (table, dirs[keep]) if return_direction else table


def render_config() -> tuple[int, int, int, int]:
    """(tile height, tile width, primitives per chunk, pixels per thread) of the render kernel."""
    import ctypes as C
    cfg = (C.c_int * 4)()
    _lib.check(_lib.load().hh_render_config(cfg))
    return tuple(cfg)


def render_host(image: np.ndarray, prims: np.ndarray, alpha: float, bgr: bool = False) -> np.ndarray:
    """hh_debug_render_host: one frame through the kernel's tile walk compiled for the host (tests; needs the library, no GPU)."""
    image = np.ascontiguousarray(image, dtype=np.uint8)
    prims = np.ascontiguousarray(prims, dtype=PRIM)
    h, w = image.shape[:2]
    desc = np.zeros(1, DESC)
    w0, w1 = blend_weights(alpha)
    desc[0] = (0, 0, h, w, 0, len(prims), w0, w1, FLAG_BGR if bgr else 0, 0)
    out = np.empty_like(image)
    _lib.check(_lib.load().hh_debug_render_host(image.ctypes.data, out.ctypes.data, desc.ctypes.data, prims.ctypes.data if len(prims) else None, len(prims)))
    return out


def render_frames_device(frames: list, tables: list, alphas, bgr=False) -> list:
    """One hh_render_poses_u8_batch, on the current stream, for a batch of frames of mixed sizes.  `frames`: uint8 RGB [h,w,3], each a
    numpy array (uploaded here) or a contiguous device tensor (read in place; the caller keeps it alive until the stream has passed
    this call).  `tables`: one build_primitives table per frame.  `alphas`, `bgr`: one value, or one per frame.  Descriptors, the
    primitive table and the pixels of the host frames travel in ONE async copy from one pinned block.
    -> list of device uint8 tensors [h,w,3], views of one allocation."""
    n = len(frames)
    if n == 0:
        return []
    alphas, bgrs = per_frame(alphas, n), per_frame(bgr, n)
    device = next((f.device for f in frames if isinstance(f, torch.Tensor)), None) or torch.device("cuda", torch.cuda.current_device())
    counts = [len(t) for t in tables]
    total_prims = int(sum(counts))
    lay = Layout()  # [descriptors | table | uploaded frames | outputs]
    lay.add(DESC.itemsize * n)
    prim_at = lay.add(PRIM.itemsize * total_prims)
    places = place_frames(lay, frames, device)
    upload = lay.pad()
    sizes = [(int(f.shape[0]), int(f.shape[1]), 3) for f in frames]
    out_at = [lay.add(h * w * 3) for h, w, _ in sizes]
    blk = Block(upload, lay.pad(), device, [f for f, at in zip(frames, places) if at is None])
    descs, prims = blk.host(0, n, DESC), blk.host(prim_at, total_prims, PRIM)
    first = 0
    for j, src in enumerate(fill_frames(blk, frames, places)):
        prims[first:first + counts[j]] = tables[j]
        w0, w1 = blend_weights(alphas[j])
        descs[j] = (src, blk.off(out_at[j]), *sizes[j][:2], first, counts[j], w0, w1, FLAG_BGR if bgrs[j] else 0, 0)
        first += counts[j]
    blk.upload()
    _lib.launch(device, _lib.load().hh_render_poses_u8_batch, blk.base, blk.addr(0), descs.ctypes.data, blk.addr(prim_at) if total_prims else None,
                prims.ctypes.data if total_prims else None, total_prims, n)
    return [blk.tensor(o, size) for o, size in zip(out_at, sizes)]


def resize_device(src: torch.Tensor, W: int, H: int) -> torch.Tensor:
    """cv2.resize(src, (W, H)) of a contiguous device uint8 [h,w] or [h,w,3] tensor on the current stream (hh_resize_u8)."""
    if not (src.dtype == torch.uint8 and src.is_cuda and src.is_contiguous() and (src.dim() == 2 or (src.dim() == 3 and src.shape[2] in (1, 3)))):
        raise ValueError("resize_device: a contiguous device uint8 [h,w], [h,w,1] or [h,w,3] tensor is needed")
    ch = 1 if src.dim() == 2 else int(src.shape[2])
    out = torch.empty((H, W) + tuple(src.shape[2:]), dtype=torch.uint8, device=src.device)
    _lib.launch(src.device, _lib.load().hh_resize_u8, src.data_ptr(), src.shape[0], src.shape[1], ch, out.data_ptr(), H, W)
    return out


def to_host(t: torch.Tensor) -> np.ndarray:
    """A finished uint8 frame back through one pinned buffer (another dtype is refused: ValueError)."""
    return frames_to_host([t])[0]


def plot_connections(image: np.ndarray, grouped_kpts_coords, grouped_kpts_scores, limbs=None, thr: float = 0.05, color_mode: str = "person",
                     alpha: float = 0.8) -> np.ndarray:
    """The reference's plot_connections (visualization.py:43-90), same signature: uploads, renders, returns uint8 [h,w,3].  Raises when
    the library or the GPU is missing."""
    if not torch.cuda.is_available():
        raise _lib.HHError("plot_connections needs the GPU: there is no CPU renderer")
    image = np.ascontiguousarray(image, dtype=np.uint8)
    table = build_primitives(grouped_kpts_coords, grouped_kpts_scores, limbs, thr, color_mode, DEFAULT_PALETTE, alpha)
    return to_host(render_frames_device([image], [table], alpha)[0])


# ---------------------------------------------------------------- heatmap panels (hh_heatmap_panels_u8)
PANEL = _lib.struct_dtype("hh_panel_map")
DIRECT, SINGLE, NESTED, AVERAGE, CLIP, MINMAX, PANEL_MAX_MAPS, PANEL_PARTS = (
    _lib.const("PANEL_" + k) for k in ("DIRECT", "SINGLE", "NESTED", "AVERAGE", "CLIP", "MINMAX", "MAX_MAPS", "PARTS"))
MEAN = (0.485, 0.456, 0.406)                   # base/transforms/base.py:5-6
STD = (0.229, 0.224, 0.225)


def jet_lut() -> np.ndarray:
    """The default colour table, uint8 [256,3] in B,G,R order as cv2.applyColorMap(arange(256), COLORMAP_JET) lists it: channel X of
    entry i is (X2 + 1) >> 1 with X2 = clamp(765 - |8 i - 510 k|, 0, 510), k = 1 (B), 2 (G), 3 (R).  A reading of OpenCV's table;
    parity with cv2 is UNPINNED (include/hhrnet.h).  The panels take any [256,3] table in its place."""
    i = np.arange(256, dtype=np.int64)[:, None]
    x2 = np.clip(765 - np.abs(8 * i - 510 * np.array([1, 2, 3], np.int64)[None, :]), 0, 510)
    return ((x2 + 1) >> 1).astype(np.uint8)


def grid_layout(n: int, nrows: int, H: int, W: int, pad: int) -> tuple[int, int, list]:
    """make_grid (utils/image.py:25-36) as bookkeeping: (grid height, grid width, [(y, x) of cell 0..n-1])."""
    if n < 1 or nrows < 1 or pad < 0:
        raise ValueError("grid_layout: need n >= 1, nrows >= 1, pad >= 0")
    ncols = -(-n // nrows)
    return (H + pad) * nrows + pad, (W + pad) * ncols + pad, [(pad + (i // ncols) * (H + pad), pad + (i % ncols) * (W + pad)) for i in range(n)]


def figure_layout(grids: list, H: int, W: int) -> tuple[list, int, int]:
    """The grids of a figure stacked vertically (np.concatenate(axis=0): all must come out equally wide).  grids: [(maps, nrows, pad)],
    maps a list of (kind, src, src2, flags).  -> ([(kind, src, src2, flags, oy, ox)], canvas height, canvas width)."""
    placed, top, width = [], 0, None
    for maps, nrows, pad in grids:
        gh, gw, at = grid_layout(len(maps), nrows, H, W, pad)
        if width not in (None, gw):
            raise ValueError("figure_layout: the grids of a figure must have one width")
        width = gw
        placed += [(kind, src, src2, flags, top + y, x) for (kind, src, src2, flags), (y, x) in zip(maps, at)]
        top += gh
    return placed, top, width


def _panel_table(placed: list, ptr) -> np.ndarray:
    table = np.zeros(len(placed), PANEL)
    for i, (kind, src, src2, flags, oy, ox) in enumerate(placed):
        table[i] = (ptr(src), ptr(src2) if src2 is not None else 0, src.shape[0], src.shape[1], kind, flags, oy, ox)
    return table


def panels_host(image: np.ndarray, placed: list, Hc: int, Wc: int, lut: np.ndarray | None = None) -> np.ndarray:
    """hh_debug_heatmap_panels_host: one figure through the kernels' arithmetic compiled for the host (tests; needs the library, no
    GPU).  placed: [(kind, src, src2, flags, oy, ox)] with float32 numpy planes."""
    image = np.ascontiguousarray(image, dtype=np.uint8)
    lut = np.ascontiguousarray(jet_lut() if lut is None else lut, dtype=np.uint8)
    keep = [(k, np.ascontiguousarray(a, np.float32), None if b is None else np.ascontiguousarray(b, np.float32), f, oy, ox) for k, a, b, f, oy, ox in placed]
    table = _panel_table(keep, lambda a: a.ctypes.data)
    out = np.empty((Hc, Wc, 3), np.uint8)
    _lib.check(_lib.load().hh_debug_heatmap_panels_host(table.ctypes.data, len(table), image.ctypes.data, image.shape[0], image.shape[1],
                                                        lut.ctypes.data, out.ctypes.data, Hc, Wc, Wc * 3))
    return out


def panels_device(image: torch.Tensor, placed: list, Hc: int, Wc: int, lut: np.ndarray | None = None, canvas: torch.Tensor | None = None,
                  pitch: int | None = None) -> torch.Tensor:
    """One hh_heatmap_panels_u8 on the current stream: every map of a figure resampled, coloured, blended over `image` (contiguous
    device uint8 [H,W,3]) and tiled, padding and unused cells zeroed.  placed: [(kind, src, src2, flags, oy, ox)], src / src2
    contiguous device float32 planes that the caller keeps alive until the stream has passed this call.  The table and the colour
    table travel in one async copy from one pinned block.  `canvas` / `pitch`: write into the caller's uint8 device buffer (row r at
    byte r * pitch of it) instead of a fresh contiguous [Hc,Wc,3].  -> the canvas."""
    if not (image.dtype == torch.uint8 and image.is_cuda and image.is_contiguous() and image.dim() == 3 and image.shape[2] == 3):
        raise ValueError("panels_device: the image must be a contiguous device uint8 [H,W,3] tensor")
    device = image.device
    H, W = int(image.shape[0]), int(image.shape[1])
    for kind, src, src2, *_ in placed:
        for t in (src,) + ((src2,) if src2 is not None else ()):
            if not (isinstance(t, torch.Tensor) and t.dtype == torch.float32 and t.device == device and t.is_contiguous() and t.dim() == 2):
                raise ValueError("panels_device: a map must be a contiguous float32 [h,w] tensor on the image's device")
    lut = np.ascontiguousarray(jet_lut() if lut is None else lut, dtype=np.uint8)
    if lut.shape != (256, 3):
        raise ValueError("panels_device: the colour table must be uint8 [256,3]")
    n = len(placed)
    lay = Layout()  # [table | colour table]
    lay.add(PANEL.itemsize * n)
    lut_at = lay.add(768)
    blk = Block(lay.end, lay.end, device)
    table = blk.host(0, n, PANEL)
    table[:] = _panel_table(placed, lambda t: t.data_ptr())
    blk.host(lut_at, 768)[:] = lut.reshape(-1)
    blk.upload()
    scratch = torch.empty(max(n, 1) * PANEL_PARTS * 2, dtype=torch.float32, device=device)
    if canvas is None:
        canvas, pitch = torch.empty((Hc, Wc, 3), dtype=torch.uint8, device=device), Wc * 3
    elif not (canvas.dtype == torch.uint8 and canvas.device == device and canvas.is_contiguous() and pitch is not None
              and canvas.numel() >= (Hc - 1) * pitch + Wc * 3):
        raise ValueError("panels_device: the canvas must be a contiguous device uint8 buffer that holds Hc rows of `pitch` bytes")
    _lib.launch(device, _lib.load().hh_heatmap_panels_u8, blk.addr(0), table.ctypes.data, n, image.data_ptr(), H, W, blk.addr(lut_at),
                canvas.data_ptr(), Hc, Wc, pitch, scratch.data_ptr())
    return canvas


def unnormalize_device(x: torch.Tensor, mean=MEAN, std=STD) -> torch.Tensor:
    """KeypointsTransform.inverse_transform (base/transforms/base.py:33-41) of a device float32 [3,H,W] tensor -> device uint8 [H,W,3]
    on the current stream (hh_unnormalize_u8)."""
    import ctypes as C
    if not (x.dtype == torch.float32 and x.is_cuda and x.dim() == 3 and x.shape[0] == 3):
        raise ValueError("unnormalize_device: a device float32 [3,H,W] tensor is needed")
    x = x.contiguous()
    out = torch.empty((x.shape[1], x.shape[2], 3), dtype=torch.uint8, device=x.device)
    _lib.launch(x.device, _lib.load().hh_unnormalize_u8, x.data_ptr(), x.shape[1], x.shape[2], (C.c_double * 3)(*mean), (C.c_double * 3)(*std),
                out.data_ptr())
    return out


def scaled_size(n: int, f: float) -> int:
    """cvRound(n * f): to nearest, half to even."""
    return int(round(float(n) * float(f)))


def resize_scaled_device(src: torch.Tensor, fx: float, fy: float) -> torch.Tensor:
    """cv2.resize(src, (0, 0), fx=fx, fy=fy) of a contiguous device uint8 [h,w] or [h,w,3] tensor on the current stream
    (hh_resize_u8_scaled)."""
    if not (src.dtype == torch.uint8 and src.is_cuda and src.is_contiguous() and (src.dim() == 2 or (src.dim() == 3 and src.shape[2] in (1, 3)))):
        raise ValueError("resize_scaled_device: a contiguous device uint8 [h,w], [h,w,1] or [h,w,3] tensor is needed")
    ch = 1 if src.dim() == 2 else int(src.shape[2])
    H, W = scaled_size(src.shape[0], fy), scaled_size(src.shape[1], fx)
    out = torch.empty((H, W) + tuple(src.shape[2:]), dtype=torch.uint8, device=src.device)
    _lib.launch(src.device, _lib.load().hh_resize_u8_scaled, src.data_ptr(), src.shape[0], src.shape[1], ch, float(fx), float(fy), out.data_ptr(), H, W)
    return out


def figure_device(image: torch.Tensor, grids: list, fx: float | None = None, lut: np.ndarray | None = None) -> torch.Tensor:
    """The grids of one figure (figure_layout) painted in one hh_heatmap_panels_u8 call, then shrunk by fx = fy (None: as painted).
    -> device uint8 [h,w,3]."""
    placed, Hc, Wc = figure_layout(grids, int(image.shape[0]), int(image.shape[1]))
    canvas = panels_device(image, placed, Hc, Wc, lut)
    return canvas if fx is None else resize_scaled_device(canvas, fx, fx)


def stack_horizontally_device(images: list, pad: int = 5) -> torch.Tensor:
    """stack_horizontally (utils/image.py:41-61) of device uint8 [h,w,3] tensors: the lower ones resized to the tallest one's height
    (hh_resize_u8), all placed side by side on a zero canvas."""
    new_h = max(int(im.shape[0]) for im in images)
    resized = [im if im.shape[0] == new_h else resize_device(im.contiguous(), int(im.shape[1] / im.shape[0] * new_h), new_h) for im in images]
    grid = torch.zeros((pad + new_h + pad, sum(int(im.shape[1]) + pad for im in resized) + pad, 3), dtype=torch.uint8, device=images[0].device)
    x = pad
    for im in resized:
        grid[pad:pad + new_h, x:x + im.shape[1]] = im
        x += int(im.shape[1]) + pad
    return grid


def plot_heatmaps(image, heatmaps, clip_0_1: bool = False, minmax: bool = False, lut: np.ndarray | None = None) -> list[np.ndarray]:
    """The reference's plot_heatmaps (visualization.py:93-110), same signature plus the colour table: image uint8 [H,W,3], heatmaps
    [K,H,W], each a numpy array (uploaded here) or a device tensor; the maps are taken as float32.  -> list of K uint8 [H,W,3].
    Raises when the library or the GPU is missing."""
    if not torch.cuda.is_available():
        raise _lib.HHError("plot_heatmaps needs the GPU: there is no CPU renderer")
    device = next((t.device for t in (image, heatmaps) if isinstance(t, torch.Tensor) and t.is_cuda), None) or torch.device("cuda", torch.cuda.current_device())
    img = (image if isinstance(image, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(image, dtype=np.uint8))).to(device).contiguous()
    hms = (heatmaps if isinstance(heatmaps, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(heatmaps, dtype=np.float32))).to(device, torch.float32).contiguous()
    if hms.dim() != 3 or tuple(hms.shape[1:]) != tuple(img.shape[:2]):
        raise ValueError("plot_heatmaps: heatmaps must be [K,H,W] with the image's H and W")
    K, H, W = hms.shape
    flags = (CLIP if clip_0_1 else 0) | (MINMAX if minmax else 0)
    out = []
    for first in range(0, K, PANEL_MAX_MAPS):
        part = hms[first:first + PANEL_MAX_MAPS]
        placed = [(DIRECT, m, None, flags, i * H, 0) for i, m in enumerate(part)]
        cells = to_host(panels_device(img, placed, len(part) * H, W, lut))
        out += [cells[i * H:(i + 1) * H] for i in range(len(part))]
    return out
