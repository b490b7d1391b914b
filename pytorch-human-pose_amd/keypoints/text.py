"""Text on the device: `put_txt` of the reference (utils/image.py:64-119), the one function through which it draws all of its text.

The host does the integer bookkeeping (`layout_put_txt`: the box, the six locs, every label's origin, one row per character), one
hh_text_labels_u8_batch launch draws the tables of a batch of frames in place, where the render and resize launches left them.  The
rule, the pixel arithmetic and the stated deviations (the font is this project's atlas, not cv2's Hershey font; primitives are
clipped to the frame) are written at hh_text_labels_u8_batch in include/hhrnet.h.  There is no CPU fallback.

The font is an atlas file that ships with the package (data/dejavu_sans_atlas.json, rasterised from DejaVu Sans by
tools/make_font_atlas.py; its licence lies beside it).  Nothing here needs FreeType.  `load_font(path)` replaces it.
"""
from __future__ import annotations

import ctypes as C
import json
import os
from decimal import Decimal

import numpy as np
import torch

from .. import _lib
from .._stage import Block, Layout

PRIM, DESC = _lib.struct_dtype("hh_render_prim"), _lib.struct_dtype("hh_render_desc")  # hh_text_prim, hh_text_desc are these
BOX, GLYPH, MAX_PRIMS = _lib.const("TEXT_BOX"), _lib.const("TEXT_GLYPH"), _lib.const("TEXT_MAX_PRIMS")
MAX_COORD = 1 << 23
GRAY, WHITE = (128, 128, 128), (255, 255, 255)  # utils/image.py:10-11
FIRST, LAST = 0x20, 0x7E
DEFAULT_FONT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "dejavu_sans_atlas.json")
LOCS = ("tl", "tc", "tr", "bl", "bc", "br")


class Font:
    """One atlas: `font_scale` [C] (the scale each size class stands for), `cap_height` [C], `glyphs` [C,95,6] (advance, bitmap
    width, bitmap height, left bearing, top relative to the baseline, offset into `coverage`), `coverage` uint8 [N]."""

    def __init__(self, path: str):
        with open(path) as fh:
            z = json.load(fh)
        self.font_scale = [Decimal(repr(float(s))) for s in z["font_scale"]]
        self.cap_height = np.array(z["cap_height"], np.int64)
        self.glyphs = np.array(z["glyphs"], np.int64)
        self.coverage = np.frombuffer(bytes.fromhex("".join(h for rows in z["coverage"] for h in rows)), np.uint8).copy()
        self.path = path
        g = self.glyphs
        if not (g.ndim == 3 and g.shape[0] == len(self.font_scale) == len(self.cap_height) and g.shape[1:] == (LAST - FIRST + 1, 6)):
            raise ValueError(f"{path}: not a font atlas (glyphs must be [classes, 95, 6])")
        if (g[..., 1:3] < 0).any() or (g[..., 1:3] > 65535).any() or (g[..., 5] < 0).any() or (g[..., 5] + g[..., 1] * g[..., 2] > len(self.coverage)).any():
            raise ValueError(f"{path}: a glyph's coverage range leaves the atlas")
        if len(self.coverage) >= 1 << 24:
            raise ValueError(f"{path}: more than 2^24 - 1 coverage bytes")
        self._device: dict = {}

    def size_class(self, font_scale: float) -> int:
        """The class whose scale is nearest to font_scale (compared as the decimals they print as), the smaller on a tie."""
        fs = Decimal(repr(float(font_scale)))
        return min(range(len(self.font_scale)), key=lambda k: (abs(self.font_scale[k] - fs), self.font_scale[k]))

    def on_device(self, device) -> torch.Tensor:
        """The coverage bytes on `device` (uploaded once per device)."""
        key = str(torch.device(device))
        if key not in self._device:
            self._device[key] = torch.from_numpy(self.coverage if len(self.coverage) else np.zeros(1, np.uint8)).to(device)
        return self._device[key]


_font: Font | None = None


def load_font(path: str | None = None) -> Font:
    """Make the atlas at `path` (None: the one that ships with the package) the font of every later call."""
    global _font
    _font = Font(path or DEFAULT_FONT)
    return _font


def font() -> Font:
    return _font or load_font()


def _codes(label: str) -> list[int]:
    """Atlas columns of a label's characters; a character outside 0x20..0x7E draws as '?'."""
    return [(ord(ch) if FIRST <= ord(ch) <= LAST else ord("?")) - FIRST for ch in label]


def _check_thickness(thickness) -> None:
    if thickness != 1:
        raise ValueError(f"thickness {thickness!r}: the atlas has one weight, only thickness=1 is drawn")


def text_size(label: str, font_scale: float = 0.5, thickness: int = 1) -> tuple[int, int]:
    """(width, height) where cv2.getTextSize(label, font, font_scale, thickness)[0] stands: the sum of the characters' integer
    advances and the cap height of font_scale's size class."""
    _check_thickness(thickness)
    f = font()
    k = f.size_class(font_scale)
    return int(f.glyphs[k, _codes(label), 0].sum()), int(f.cap_height[k])


def _clip(x0: int, y0: int, x1: int, y1: int, img_h: int, img_w: int) -> tuple:
    """An inclusive rectangle clipped to the frame; (0, 0, -1, -1) when nothing is left."""
    x0, y0, x1, y1 = max(x0, 0), max(y0, 0), min(x1, img_w - 1), min(y1, img_h - 1)
    return (x0, y0, x1, y1) if x0 <= x1 and y0 <= y1 else (0, 0, -1, -1)


def layout_put_txt(img_h: int, img_w: int, labels: list, vspace: int = 10, font_scale: float = 0.5, thickness: int = 1, loc: str = "tl",
                   bg_color=GRAY, txt_color=WHITE, alpha: float = 1.0, bgr: bool = False, return_layout: bool = False):
    """put_txt's arithmetic (utils/image.py:76-118) in integers -> the rows of one call in draw order (structured array of
    hh_text_prim): one BOX, then one GLYPH per character that has ink.  Tables of several calls concatenate (np.concatenate) into
    one that composes them in order.  Colours are stored as given, in the frame's own channel order, as cv2 applies them; `bgr`: the
    frame is stored B,G,R and the colours are given as R,G,B (they are reversed here).
    `return_layout`: also dict(box=(x0, y0, x1, y1) inclusive and unclipped, opaque, weights=(1 - alpha, alpha) in double,
    bg_color, txt_color, origins=[(x, y) baseline-left of every label], size_class)."""
    _check_thickness(thickness)
    alpha = float(alpha)
    if not np.isfinite(alpha):
        raise ValueError("alpha must be finite")
    if loc not in LOCS:
        raise ValueError(f"loc {loc!r} is not one of {LOCS}")
    img_h, img_w, vspace = int(img_h), int(img_w), int(vspace)
    f = font()
    k = f.size_class(font_scale)
    height = int(f.cap_height[k])
    codes = [_codes(str(label)) for label in labels]
    txt_h = vspace + len(codes) * (height + vspace)
    txt_w = max([0] + [int(f.glyphs[k, c, 0].sum()) for c in codes]) + 2 * vspace
    y = vspace if loc[0] == "t" else img_h - txt_h + vspace
    x = {"l": vspace, "r": img_w - txt_w + vspace, "c": img_w // 2 - txt_w // 2 + vspace // 2}[loc[1]]
    _x, _y = x - vspace, y - vspace
    opaque = not alpha < 1
    # alpha < 1: the slice [_y : _y + txt_h, _x : _x + txt_w]; otherwise cv2.rectangle to (_x + txt_w, _y + txt_h), inclusive
    box = (_x, _y, _x + txt_w - (0 if opaque else 1), _y + txt_h - (0 if opaque else 1))
    bg, fg = (tuple(int(v) for v in tuple(c)[:3][::-1 if bgr else 1]) for c in (bg_color, txt_color))
    if max(abs(v) for v in box) > MAX_COORD:
        raise ValueError("text box beyond +-2^23")
    rows = [(0, 0, 1 if opaque else 0, 0, 0.0 if opaque else np.float32(1.0 - alpha), 1.0 if opaque else np.float32(alpha), bg, BOX,
             *_clip(*box, img_h, img_w))]
    origins = []
    for c in codes:
        origins.append((x, y + height))
        pen = x
        for adv, w, h, left, top, off in f.glyphs[k, c].tolist():
            if w and h:
                cx, cy = pen + left, y + height + top
                if max(abs(cx), abs(cy)) > MAX_COORD:
                    raise ValueError("glyph beyond +-2^23")
                rows.append((cx, cy, w, h, float(off), 0.0, fg, GLYPH, *_clip(cx, cy, cx + w - 1, cy + h - 1, img_h, img_w)))
            pen += adv
        y += height + vspace
    table = np.zeros(len(rows), PRIM)
    for n, row in enumerate(rows):
        table[n] = row
    if return_layout:
        return table, dict(box=box, opaque=opaque, weights=(1.0 - alpha, alpha), bg_color=bg, txt_color=fg, origins=origins, size_class=k)
    return table


def video_labels(idx: int, num_frames: int, model_input_shape, speed_ms: dict) -> list[str]:
    """The strings InferenceVideoDataset.draw_labels (base/datasets/video.py:168-176) writes on a frame."""
    input_h, input_w = model_input_shape
    return [f"{idx} / {num_frames}", f"Model input shape: {input_h} x {input_w}", "Latency [ms]: "] + [f"  {name}: {value}" for name, value in speed_ms.items()]


def video_table(img_h: int, img_w: int, labels: list) -> np.ndarray:
    """draw_labels' put_txt call: loc="tl", alpha=0.6, font_scale=0.5 (grey and white: the same in R,G,B and B,G,R)."""
    return layout_put_txt(img_h, img_w, labels, loc="tl", alpha=0.6, font_scale=0.5)


def text_config() -> tuple[int, int, int, int]:
    """(tile height, tile width, primitives per chunk, pixels per thread) of the text kernel."""
    cfg = (C.c_int * 4)()
    _lib.check(_lib.load().hh_text_config(cfg))
    return tuple(cfg)


def put_txt_host(image: np.ndarray, table: np.ndarray) -> np.ndarray:
    """hh_debug_text_host: one frame through the kernel's tile walk compiled for the host (tests; needs the library, no GPU).
    -> a drawn copy of `image`."""
    out = np.array(image, dtype=np.uint8, order="C")
    if out.ndim != 3 or out.shape[2] != 3:
        raise ValueError("put_txt_host: a uint8 [h,w,3] image is needed")
    table = np.ascontiguousarray(table, dtype=PRIM)
    desc = np.zeros(1, DESC)
    desc[0] = (0, 0, out.shape[0], out.shape[1], 0, len(table), 0.0, 0.0, 0, 0)
    atlas = font().coverage
    _lib.check(_lib.load().hh_debug_text_host(out.ctypes.data, desc.ctypes.data, table.ctypes.data if len(table) else None, len(table), atlas.ctypes.data,
                                              len(atlas)))
    return out


def stage_put_txt(frames: list, tables: list):
    """Everything of put_txt_device in front of the launch: the validation on the host copies and the ONE async copy of descriptors,
    table and tile list from one pinned block.  -> a function that enqueues the launch on the current stream (tools/text_time.py
    times it alone; its `num_tiles` is the length of the tile list), or None when no primitive touches a frame."""
    n = len(frames)
    if len(tables) != n:
        raise ValueError("put_txt_device: one table per frame")
    if n == 0:
        return None
    device = frames[0].device
    for f in frames:
        if not (isinstance(f, torch.Tensor) and f.dtype == torch.uint8 and f.is_cuda and f.is_contiguous() and f.dim() == 3 and f.shape[2] == 3
                and f.device == device):
            raise ValueError("put_txt_device: a frame must be a contiguous uint8 [h,w,3] tensor, all on one device")
    lib = _lib.load()
    fnt = font()
    atlas = fnt.on_device(device)
    counts = [len(t) for t in tables]
    total = int(sum(counts))
    prims = np.concatenate([np.ascontiguousarray(t, dtype=PRIM) for t in tables]) if total else np.zeros(0, PRIM)
    descs = np.zeros(n, DESC)
    first = 0
    for j, f in enumerate(frames):  # (the frames' offsets need the block's address: the tile list does not read them)
        descs[j] = (0, 0, f.shape[0], f.shape[1], first, counts[j], 0.0, 0.0, 0, 0)
        first += counts[j]
    num_tiles = C.c_longlong(0)
    args = (descs.ctypes.data, prims.ctypes.data if total else None, total, n, len(fnt.coverage))
    _lib.check(lib.hh_text_tiles(*args, None, 0, C.byref(num_tiles)))
    nt = num_tiles.value
    if nt == 0:
        return None
    lay = Layout()  # [descriptors | table | tile list]
    lay.add(DESC.itemsize * n)
    prim_at = lay.add(PRIM.itemsize * total)
    tile_at = lay.add(8 * nt)
    blk = Block(lay.end, lay.end, device, frames)
    descs["src_offset"] = descs["dst_offset"] = [blk.off_of(f) for f in frames]
    blk.host(0, DESC.itemsize * n)[:] = descs.view(np.uint8)  # (as bytes: a structured assignment goes field by field)
    blk.host(prim_at, PRIM.itemsize * total)[:] = prims.view(np.uint8)
    tiles = blk.host(tile_at, 8 * nt)
    _lib.check(lib.hh_text_tiles(*args, tiles.ctypes.data, nt, C.byref(num_tiles)))
    blk.upload()

    def launch():  # (the block keeps the frames, the device bytes and the host copies alive)
        _lib.launch(device, lib.hh_text_labels_u8_batch, blk.base, blk.addr(0), descs.ctypes.data, blk.addr(prim_at), prims.ctypes.data, total, n,
                    atlas.data_ptr(), len(fnt.coverage), blk.addr(tile_at), tiles.ctypes.data, nt)
        return frames
    launch.num_tiles = nt
    return launch


def put_txt_device(frames: list, tables: list) -> list:
    """One hh_text_labels_u8_batch on the current stream: frame j, a contiguous device uint8 [h,w,3] tensor, gets tables[j] (rows
    of layout_put_txt, several calls concatenated in order) drawn IN PLACE.  Descriptors, table and tile list travel in ONE async
    copy from one pinned block; everything is validated on the host copies before the launch.  -> `frames`."""
    launch = stage_put_txt(frames, tables)
    if launch is not None:
        launch()
    return frames


def put_txt(image, labels: list, vspace: int = 10, font=None, font_scale: float = 0.5, thickness: int = 1, loc: str = "tl", bg_color=GRAY,
            txt_color=WHITE, alpha: float = 1.0):
    """The reference's put_txt, same signature and defaults (`font` is accepted and ignored: there is one font, load_font's).
    `image`: a uint8 [h,w,3] numpy array (uploaded, drawn, copied back into it) or a contiguous device tensor (drawn in place).
    -> `image`, as the reference returns it.  Raises when the library or the GPU is missing."""
    table = layout_put_txt(image.shape[0], image.shape[1], labels, vspace, font_scale, thickness, loc, bg_color, txt_color, alpha)
    if isinstance(image, torch.Tensor):
        put_txt_device([image], [table])
        return image
    if not torch.cuda.is_available():
        raise _lib.HHError("put_txt needs the GPU: there is no CPU renderer")
    if not (isinstance(image, np.ndarray) and image.dtype == np.uint8 and image.ndim == 3 and image.shape[2] == 3):
        raise ValueError("put_txt: a uint8 [h,w,3] image is needed")
    from .visualization import to_host
    frame = torch.from_numpy(np.ascontiguousarray(image)).to(torch.device("cuda", torch.cuda.current_device()))
    np.copyto(image, to_host(put_txt_device([frame], [table])[0]))
    return image
