"""Dataset sample figures on the device: `plot_raw`, `plot` and `plot_examples` of the reference's CocoKeypointsDataset
(keypoints/datasets/coco.py:377-449, base/datasets/base.py:55-58), the figure its DatasetExamplesCallback logs at on_fit_start, from
data that `TrainInput` built on the device.

The host does the bookkeeping as plain data (`seg_tables`, `plan_raw`, `plan_sample`: which polygons in which colours, the skeleton
primitives, the letterbox, every text table, every cell's place); the pixels are launches: hh_render_poses_u8_batch (skeletons),
hh_seg_overlay_u8_batch (the per-object segmentation overlay of the raw pane, new with this module), hh_resize_u8,
hh_unnormalize_u8, hh_heatmap_panels_u8 with HH_PANEL_DIRECT (target heatmaps), hh_text_labels_u8_batch (put_txt).  Only the finished
uint8 figure is copied back.  There is no CPU renderer.

What is pinned where (the rules themselves are written in include/hhrnet.h):
  * to the reference, by tests/golden/sample_plot.npz: the polygons as cv2 would receive them, their order and colours, the blend weights,
    the skeleton calls, the letterbox parameters as restated below, every put_txt call, the plot_heatmaps inputs, the grid placements,
    the final size;
  * to the header's text: the fill and line rasterisation, the blend, the resize, the fonts, the JET table;
  * UNPINNED for want of cv2 and albumentations: cv2.fillPoly / drawContours boundary pixels, albumentations' LongestMaxSize +
    PadIfNeeded (restated in `letterbox`), cv2.resize, cv2's fonts, the JET table.
Stated deviation: a run-length (iscrowd) segmentation is drawn as one fill without contour; the reference first turns it into polygons
with cv2.findContours.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from .. import _lib
from .._stage import Block, Layout, fill_frames, per_frame, place_frames
from . import crowd_mask as cm
from . import text as tx
from . import visualization as vis
from .visualization import DEFAULT_PALETTE

DESC = vis.DESC  # hh_seg_desc IS hh_render_desc
SHAPE_INTS, MAX_SHAPES = _lib.const("SEG_SHAPE_INTS"), _lib.const("SEG_MAX_SHAPES")
FILL, LINE = _lib.const("SEG_FILL"), _lib.const("SEG_LINE")
MAX_COORD = 1 << 23
OVERLAY_ALPHA = 0.4  # coco.py:395
COCO_LABELS = ["nose", "left_eye", "right_eye", "left_ear", "right_ear", "left_shoulder", "right_shoulder", "left_elbow", "right_elbow",
               "left_wrist", "right_wrist", "left_hip", "right_hip", "left_knee", "right_knee", "left_ankle", "right_ankle"]  # coco.py:25-43
COCO_LIMBS = [(9, 7), (7, 5), (5, 3), (3, 1), (1, 0), (0, 2), (1, 2), (2, 4), (4, 6), (6, 8), (8, 10), (5, 6), (5, 11), (6, 12), (11, 12),
              (11, 13), (13, 15), (12, 14), (14, 16)]  # coco.py:45-65


# ---------------------------------------------------------------------------------------------------------------- host half (no GPU)
def polygon_vertices(poly) -> np.ndarray:
    """np.array(poly).reshape(-1, 2).astype(np.int32) (coco.py:391): truncation toward zero; an odd count raises ValueError."""
    return np.array(poly).reshape(-1, 2).astype(np.int32)


def _column_range(t: np.ndarray, h: int, w: int) -> tuple[int, int]:
    if t.size == 0:
        return 0, 0
    first = min(int(t[0]) // h, w - 1)
    return first, (w - 1 if t.size & 1 else max((int(t[-1]) - 1) // h, first))


def seg_tables(annot, h: int, w: int, palette=DEFAULT_PALETTE, shift: float = 0.5):
    """The overlay tables of one frame in the reference's order (coco.py:385-393) -> (shapes int32 [n,8], toggles uint32 [m]).
    Object i, in annotation order, is drawn in palette[i] (more objects than palette entries raise IndexError, as get_color does).  Each
    polygon of its `segmentation`, in order: one FILL row, then its closed contour as LINE rows vertex j -> j + 1, last -> first.  The
    fill's toggles are hh_crowd_polygon_toggles of the truncated vertices plus `shift` = 0.5 in both coordinates (an integer vertex is a
    pixel centre, cv2's convention; COCO's rule samples centres at +0.5).  A polygon of fewer than 3 vertices gives its LINE rows only.
    A run-length dict gives one FILL row from crowd_mask.rle_toggles and no contour."""
    h, w = int(h), int(w)
    palette = np.asarray(palette)
    rows, toggles, at = [], [], 0

    def fill(t: np.ndarray, colour: int) -> None:
        nonlocal at
        rows.append((FILL, colour, at, t.size, *_column_range(t, h, w), 0, 0))
        toggles.append(t.astype(np.uint32))
        at += t.size

    for i, obj in enumerate(annot):
        if i >= len(palette):
            raise IndexError(f"palette of {len(palette)} colours, object {i} needs one more")
        r, g, b = (int(v) for v in palette[i][:3])
        colour = r | g << 8 | b << 16
        seg = obj["segmentation"]
        if isinstance(seg, dict):
            if [int(v) for v in seg["size"]] != [h, w]:
                raise ValueError(f"run-length size {seg['size']} differs from the image {[h, w]}")
            fill(cm.rle_toggles(seg["counts"], h, w), colour)
            continue
        for poly in seg:
            v = polygon_vertices(poly)
            if len(v) and np.abs(v.astype(np.int64)).max() > MAX_COORD:
                raise ValueError("polygon vertex beyond +-2^23")
            if len(v) >= 3:
                fill(cm.polygon_toggles((v.astype(np.float64) + shift).reshape(-1), h, w), colour)
            for j in range(len(v)):
                (xa, ya), (xb, yb) = v[j], v[(j + 1) % len(v)]
                rows.append((LINE, colour, int(xa), int(ya), int(xb), int(yb), 0, 0))
    shapes = np.array(rows, np.int32).reshape(-1, SHAPE_INTS)
    return shapes, (np.concatenate(toggles) if toggles else np.zeros(0, np.uint32))


def recorded_polygons(shapes: np.ndarray) -> list:
    """The overlay table read back as the reference's cv2 calls: [(colour (r, g, b), vertices [k,2])] per polygon, from the LINE rows
    (a closed contour ends where its last row returns to its first vertex)."""
    out, cur, colour = [], [], None
    for kind, col, a, b, c, d, *_ in np.asarray(shapes).tolist():
        if kind != LINE:
            continue
        if not cur:
            colour = (col & 255, col >> 8 & 255, col >> 16 & 255)
        cur.append((a, b))
        if (c, d) == cur[0]:
            out.append((colour, np.array(cur, np.int32)))
            cur = []
    return out


def annot_joints(annot, num_kpts: int = 17) -> np.ndarray:
    """get_coco_joints (coco.py:68-74) over ALL objects, as plot_raw takes them."""
    joints = np.zeros((len(annot), num_kpts, 3))
    for i, obj in enumerate(annot):
        joints[i] = np.array(obj["keypoints"]).reshape([-1, 3])
    return joints


def letterbox(h: int, w: int, max_size: int) -> tuple[int, int, int, int]:
    """A.LongestMaxSize(max_size) then A.PadIfNeeded(max_size, max_size, BORDER_CONSTANT) restated (UNPINNED: albumentations is not
    available where this is built): new side = rint_half_even(side * (max_size / max(h, w))) in float64; zero padding with
    top = (max_size - new_h) // 2, left likewise, the remainder below and to the right.  -> (new_h, new_w, top, left)."""
    scale = max_size / max(h, w)
    new_h, new_w = int(round(h * scale)), int(round(w * scale))
    if not (1 <= new_h <= max_size and 1 <= new_w <= max_size):
        raise ValueError(f"letterbox: a {h} x {w} image does not fit {max_size}")
    return new_h, new_w, (max_size - new_h) // 2, (max_size - new_w) // 2


def plan_raw(h: int, w: int, annot, max_size: int, limbs=COCO_LIMBS, palette=DEFAULT_PALETTE) -> dict:
    """plot_raw (coco.py:377-410) as plain data: the skeleton primitives of all objects' keypoints (thr 0.5, person colours, alpha
    0.8), the overlay tables and weights, the letterbox, the put_txt table of the finished pane."""
    joints = annot_joints(annot)
    shapes, toggles = seg_tables(annot, h, w, palette)
    new_h, new_w, top, left = letterbox(h, w, max_size)
    labels = ["Raw Image", f"Shape: {h} x {w}"]
    return dict(size=(int(max_size), int(max_size)), raw_size=(int(h), int(w)),
                prims=vis.build_primitives(joints[..., :2], joints[..., 2], limbs, 0.5, "person", palette), skeleton_alpha=0.8,
                shapes=shapes, toggles=toggles, overlay_alpha=OVERLAY_ALPHA, weights=vis.blend_weights(OVERLAY_ALPHA),
                letterbox=(new_h, new_w, top, left), labels=labels, text=tx.layout_put_txt(max_size, max_size, labels))


def _shift(table: np.ndarray, oy: int, ox: int) -> np.ndarray:
    """A put_txt table laid out for a cell, moved to the cell's origin inside a canvas (its boxes were clipped to the cell)."""
    t = table.copy()
    for f, o in (("cx", ox), ("x0", ox), ("x1", ox), ("cy", oy), ("y0", oy), ("y1", oy)):
        t[f] += o
    return t


def plan_sample(raw_hw, annot, stage_sizes, joints_list, filename: str, labels=COCO_LABELS, limbs=COCO_LIMBS, nrows: int = 3, stage_idxs=(1,),
                palette=DEFAULT_PALETTE) -> dict:
    """plot (coco.py:412-449) as plain data.  stage_sizes[i] = (h, w) of stage i's maps, joints_list[i] its integer joints [P,K,3] (x, y,
    visibility).  Per plotted stage: the skeleton primitives (thr 0.5), the put_txt calls (cell, labels, alpha, font_scale) with their
    tables moved to the cell's place in the stage grid, the cells' places (image, crowd mask, one per keypoint), the grid's size; then
    the size all stage grids are resized to and their places in the model-input grid, the raw pane (plan_raw at that grid's height),
    the horizontal stack and the final size."""
    K = len(labels)
    stages = []
    for idx in stage_idxs:
        h, w = (int(v) for v in stage_sizes[idx])
        joints = np.asarray(joints_list[idx], np.float64).reshape(-1, K, 3)
        gh, gw, cells = vis.grid_layout(2 + K, nrows, h, w, 5)
        if idx == 1:
            font_scale, image_labels = 0.5, ["Transformed Image", f"Sample: {filename}", f"Stage: {idx} ({h} x {w})"]
        else:
            font_scale, image_labels = 0.25, [f"Stage: {idx} ({h} x {w})"]
        calls = []  # (cell, labels, alpha, font_scale) in the reference's order
        if idx == 1:
            calls += [(2 + i, [labels[i]], 0.8, font_scale) for i in range(K)]
            calls.append((1, ["Crowd Mask"], 1, font_scale))
        calls.append((0, image_labels, 0.8, font_scale))
        tables = [_shift(tx.layout_put_txt(h, w, lab, alpha=alpha, font_scale=fs), *cells[cell]) for cell, lab, alpha, fs in calls]
        stages.append(dict(stage=int(idx), size=(h, w), grid=(gh, gw), cells=cells, text_calls=calls,
                           prims=vis.build_primitives(joints[..., :2], joints[..., 2], limbs, 0.5, "person", palette), skeleton_alpha=0.8,
                           text=np.concatenate(tables) if tables else np.zeros(0, tx.PRIM)))
    mh, mw = max(s["grid"][0] for s in stages), max(s["grid"][1] for s in stages)
    Gh, Gw, places = vis.grid_layout(len(stages), len(stages), mh, mw, 5)
    raw = plan_raw(int(raw_hw[0]), int(raw_hw[1]), annot, Gh, limbs, palette)
    pad = 5  # stack_horizontally: both panes are Gh high, nothing is resized
    return dict(stages=stages, matched=(mh, mw), model_grid=(Gh, Gw), model_places=places, raw=raw,
                stack=[(pad, pad), (pad, pad + Gh + pad)], size=(pad + Gh + pad, pad + Gh + pad + Gw + pad))


def plan_examples(sample_sizes, pad: int = 20) -> dict:
    """plot_examples (base.py:55-58): make_grid(plots, nrows=len(plots), pad=20) -> the places and the final size."""
    sizes = [tuple(int(v) for v in s) for s in sample_sizes]
    if len(set(sizes)) != 1:
        raise ValueError("plot_examples: the sample figures must be equally large (make_grid)")
    H, W, places = vis.grid_layout(len(sizes), len(sizes), *sizes[0], pad)
    return dict(places=places, size=(H, W))


# ---------------------------------------------------------------------------------------------------------------- the overlay launch
def overlay_config() -> tuple[int, int, int, int]:
    """(tile rows, tile columns, threads per workgroup, shapes culled per chunk) of the overlay kernel."""
    cfg = (C.c_int * 4)()
    _lib.check(_lib.load().hh_seg_overlay_config(cfg))
    return tuple(cfg)


def _tables(shapes, toggles) -> tuple[np.ndarray, np.ndarray]:
    return (np.ascontiguousarray(np.asarray(shapes, np.int32).reshape(-1, SHAPE_INTS)), np.ascontiguousarray(np.asarray(toggles, np.uint32).reshape(-1)))


def overlay_host(image: np.ndarray, shapes, toggles, alpha: float = OVERLAY_ALPHA, bgr: bool = False, in_place: bool = False) -> np.ndarray:
    """hh_debug_seg_overlay_host: one frame through the kernel's tile walk compiled for the host (tests; needs the library, no GPU)."""
    image = np.array(image, dtype=np.uint8, order="C")
    shapes, toggles = _tables(shapes, toggles)
    w0, w1 = vis.blend_weights(alpha)
    desc = np.zeros(1, DESC)
    desc[0] = (0, 0, image.shape[0], image.shape[1], 0, len(shapes), w0, w1, vis.FLAG_BGR if bgr else 0, 0)
    out = image if in_place else np.empty_like(image)
    _lib.check(_lib.load().hh_debug_seg_overlay_host(image.ctypes.data, out.ctypes.data, desc.ctypes.data, shapes.ctypes.data if len(shapes) else None, len(shapes),
                                                     toggles.ctypes.data if len(toggles) else None, len(toggles)))
    return out


def stage_overlay(frames: list, tables: list, alphas=OVERLAY_ALPHA, bgr=False, in_place: bool = False):
    """Everything of overlay_frames_device in front of the launch: the tables and the ONE async copy of descriptors, shapes, toggles and
    host frames from one pinned block.  -> a function that enqueues the launch on the current stream and returns the output tensors
    (tools/sample_plot_time.py times it alone), or None for no frames."""
    n = len(frames)
    if n == 0:
        return None
    if len(tables) != n:
        raise ValueError("overlay_frames_device: one (shapes, toggles) per frame")
    lib = _lib.load()
    alphas, bgrs = per_frame(alphas, n), per_frame(bgr, n)
    device = next((f.device for f in frames if isinstance(f, torch.Tensor)), None) or torch.device("cuda", torch.cuda.current_device())
    tabs = [_tables(*t) for t in tables]
    num_shapes, num_toggles = sum(len(s) for s, _ in tabs), sum(len(t) for _, t in tabs)
    lay = Layout()  # [descriptors | shapes | toggles | uploaded frames | outputs]
    lay.add(DESC.itemsize * n)
    shape_at = lay.add(4 * SHAPE_INTS * num_shapes)
    toggle_at = lay.add(4 * num_toggles)
    places = place_frames(lay, frames, device)
    upload = lay.pad()
    sizes = [(int(f.shape[0]), int(f.shape[1]), 3) for f in frames]
    # in place: an uploaded frame is overwritten where it was uploaded to, a device frame where it lies (None)
    out_at = places if in_place else [lay.add(h * w * 3) for h, w, _ in sizes]
    blk = Block(upload, lay.pad(), device, [f for f, at in zip(frames, places) if at is None])
    descs = blk.host(0, n, DESC)
    shapes = blk.host(shape_at, SHAPE_INTS * num_shapes, np.int32).reshape(-1, SHAPE_INTS)
    toggles = blk.host(toggle_at, num_toggles, np.uint32)
    first = tog = 0
    for j, (src, (s, t)) in enumerate(zip(fill_frames(blk, frames, places), tabs)):
        shapes[first:first + len(s)] = s
        fills = shapes[first:first + len(s)]
        fills[fills[:, 0] == FILL, 2] += tog  # a fill's first toggle counts from the batch's table
        toggles[tog:tog + len(t)] = t
        w0, w1 = vis.blend_weights(alphas[j])
        descs[j] = (src, src if in_place else blk.off(out_at[j]), *sizes[j][:2], first, len(s), w0, w1, vis.FLAG_BGR if bgrs[j] else 0, 0)
        first += len(s)
        tog += len(t)
    blk.upload()
    outs = [f if o is None else blk.tensor(o, size) for f, o, size in zip(frames, out_at, sizes)]

    def launch():  # (the block keeps the frames, the device bytes and the host copies alive)
        _lib.launch(device, lib.hh_seg_overlay_u8_batch, blk.base, blk.addr(0), descs.ctypes.data, blk.addr(shape_at) if num_shapes else None,
                    shapes.ctypes.data if num_shapes else None, num_shapes, blk.addr(toggle_at) if num_toggles else None,
                    toggles.ctypes.data if num_toggles else None, num_toggles, n)
        return outs
    launch.num_shapes, launch.num_toggles = num_shapes, num_toggles
    return launch


def overlay_frames_device(frames: list, tables: list, alphas=OVERLAY_ALPHA, bgr=False, in_place: bool = False) -> list:
    """One hh_seg_overlay_u8_batch, on the current stream, for a batch of frames of mixed sizes.  `frames`: uint8 RGB [h,w,3], each a
    numpy array (uploaded here) or a contiguous device tensor (read where it lies).  `tables`: one (shapes, toggles) of seg_tables per
    frame.  `alphas`, `bgr`: one value, or one per frame.  Descriptors, both tables and the pixels of the host frames travel in ONE
    async copy from one pinned block; everything is validated on the host copies before the launch.  `in_place`: device frames are
    overwritten and returned themselves.  -> list of device uint8 tensors [h,w,3]."""
    launch = stage_overlay(frames, tables, alphas, bgr, in_place)
    return launch() if launch is not None else []


# ---------------------------------------------------------------------------------------------------------------- the figures
def _need_gpu(what: str) -> None:
    if not torch.cuda.is_available():
        raise _lib.HHError(f"{what} needs the GPU: there is no CPU renderer")


def _frame(image, device=None) -> torch.Tensor:
    """A uint8 [h,w,3] numpy array, device tensor or jpeg.JpegImage -> a contiguous device tensor."""
    from . import jpeg as jp
    if isinstance(image, jp.JpegImage):
        return jp.decode_jpeg_device([image], device=device)[0].contiguous()
    if isinstance(image, torch.Tensor):
        if not (image.is_cuda and image.dtype == torch.uint8 and image.dim() == 3 and image.shape[2] == 3):
            raise ValueError("a device image must be a uint8 [h,w,3] tensor")
        return image.contiguous()
    image = np.ascontiguousarray(image)
    if not (image.dtype == np.uint8 and image.ndim == 3 and image.shape[2] == 3):
        raise ValueError("a uint8 [h,w,3] image is needed")
    return torch.from_numpy(image).to(device or torch.device("cuda", torch.cuda.current_device()))


def plot_segmentations_device(image, annot, alpha: float = OVERLAY_ALPHA, palette=DEFAULT_PALETTE) -> torch.Tensor:
    """The overlay step of plot_raw alone (coco.py:383-398) -> device uint8 [h,w,3]."""
    _need_gpu("plot_segmentations")
    frame = _frame(image)
    return overlay_frames_device([frame], [seg_tables(annot, frame.shape[0], frame.shape[1], palette)], alpha)[0]


def plot_segmentations(image, annot, alpha: float = OVERLAY_ALPHA) -> np.ndarray:
    return vis.to_host(plot_segmentations_device(image, annot, alpha))


def _draw_raw(frame: torch.Tensor, plan: dict) -> torch.Tensor:
    """plan_raw's launches: skeletons, overlay, resize, the zero-padded square, the labels."""
    drawn = vis.render_frames_device([frame], [plan["prims"]], plan["skeleton_alpha"])[0]
    drawn = overlay_frames_device([drawn], [(plan["shapes"], plan["toggles"])], plan["overlay_alpha"], in_place=True)[0]
    new_h, new_w, top, left = plan["letterbox"]
    if (new_h, new_w) != tuple(drawn.shape[:2]):
        drawn = vis.resize_device(drawn, new_w, new_h)
    pane = torch.zeros((*plan["size"], 3), dtype=torch.uint8, device=frame.device)
    pane[top:top + new_h, left:left + new_w] = drawn
    return tx.put_txt_device([pane], [plan["text"]])[0]


def plot_raw_device(image, annot, max_size: int, limbs=COCO_LIMBS) -> torch.Tensor:
    """plot_raw (coco.py:377-410) -> device uint8 [max_size, max_size, 3]."""
    _need_gpu("plot_raw")
    frame = _frame(image)
    return _draw_raw(frame, plan_raw(frame.shape[0], frame.shape[1], annot, max_size, limbs))


def plot_raw(image, annot, max_size: int, limbs=COCO_LIMBS) -> np.ndarray:
    return vis.to_host(plot_raw_device(image, annot, max_size, limbs))


def _to_device(t, device, dtype) -> torch.Tensor:
    return (t if isinstance(t, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(t))).to(device, dtype).contiguous()


def plot_sample_device(image, annot, sample, filename: str, labels=COCO_LABELS, limbs=COCO_LIMBS, nrows: int = 3, stage_idxs=(1,)) -> torch.Tensor:
    """plot (coco.py:412-449) of one sample -> device uint8 figure.  `image`, `annot`: the raw image and its annotation (the raw pane);
    `sample` = (img [3,S,S] normalised, [heatmaps [K,s,s]], [mask [s,s]], [int joints [P,K,3]]): one sample's slices of a batch, numpy
    or device tensors."""
    _need_gpu("plot_sample")
    frame = _frame(image)
    device = frame.device
    img, heatmaps, masks, joints_list = sample
    plan = plan_sample(frame.shape[:2], annot, [tuple(m.shape[-2:]) for m in masks], joints_list, filename, labels, limbs, nrows, stage_idxs)
    img_u8 = vis.unnormalize_device(_to_device(img, device, torch.float32))  # KeypointsTransform.inverse_transform
    grids = []
    for st in plan["stages"]:
        idx, (h, w), (gh, gw), cells = st["stage"], st["size"], st["grid"], st["cells"]
        small = img_u8 if (h, w) == tuple(img_u8.shape[:2]) else vis.resize_device(img_u8, w, h)
        hms = _to_device(heatmaps[idx], device, torch.float32)
        placed = [(vis.DIRECT, hms[k], None, 0, *cells[2 + k]) for k in range(hms.shape[0])]
        grid = vis.panels_device(small, placed, gh, gw)  # zero but for the heatmap cells
        (y0, x0), (y1, x1) = cells[0], cells[1]
        grid[y0:y0 + h, x0:x0 + w] = vis.render_frames_device([small], [st["prims"]], st["skeleton_alpha"])[0]
        mask = (_to_device(masks[idx], device, torch.float32) * 255).to(torch.uint8)  # (crowd_mask * 255).astype(np.uint8)
        grid[y1:y1 + h, x1:x1 + w] = mask[:, :, None]
        grids.append(tx.put_txt_device([grid], [st["text"]])[0])
    mh, mw = plan["matched"]
    model = torch.zeros((*plan["model_grid"], 3), dtype=torch.uint8, device=device)
    for g, (y, x) in zip(grids, plan["model_places"]):
        model[y:y + mh, x:x + mw] = g if tuple(g.shape[:2]) == (mh, mw) else vis.resize_device(g, mw, mh)
    raw = _draw_raw(frame, plan["raw"])
    out = vis.stack_horizontally_device([raw, model])
    assert tuple(out.shape[:2]) == plan["size"]
    return out


def plot_sample(image, annot, sample, filename: str, labels=COCO_LABELS, limbs=COCO_LIMBS, nrows: int = 3, stage_idxs=(1,)) -> np.ndarray:
    return vis.to_host(plot_sample_device(image, annot, sample, filename, labels, limbs, nrows, stage_idxs))


def plot_examples_device(items, nrows: int = 1, stage_idxs=(1, 0), labels=COCO_LABELS, limbs=COCO_LIMBS) -> torch.Tensor:
    """plot_examples (coco.py:372-375, base.py:55-58): items = [(image, annot, sample, filename)] -> make_grid(plots, nrows=len(plots),
    pad=20) of plot_sample over them, on the device."""
    plots = [plot_sample_device(image, annot, sample, filename, labels, limbs, nrows, stage_idxs) for image, annot, sample, filename in items]
    if not plots:
        raise ValueError("plot_examples: at least one item")
    plan = plan_examples([p.shape[:2] for p in plots])
    grid = torch.zeros((*plan["size"], 3), dtype=torch.uint8, device=plots[0].device)
    for p, (y, x) in zip(plots, plan["places"]):
        grid[y:y + p.shape[0], x:x + p.shape[1]] = p
    return grid


def plot_examples(items, nrows: int = 1, stage_idxs=(1, 0), labels=COCO_LABELS, limbs=COCO_LIMBS) -> np.ndarray:
    return vis.to_host(plot_examples_device(items, nrows, stage_idxs, labels, limbs))


def plot_examples_jpeg(items, nrows: int = 1, stage_idxs=(1, 0), quality: int = 90, subsampling="420") -> bytes:
    """The same figure as one JFIF stream, encoded on the device (jpeg.encode_jpeg_device)."""
    from . import jpeg as jp
    return jp.encode_jpeg_device([plot_examples_device(items, nrows, stage_idxs)], quality, subsampling)[0]
