"""The input of the training step built on the device: augmentation warps, crowd masks and target heatmaps.

Stands in for what the reference's dataset worker does per sample on the host (`src/keypoints/transforms.py:75-172`
RandomAffineTransform, `:56-72` RandomHorizontalFlip, `:37-53` ToTensor + Normalize; `src/keypoints/datasets/coco.py:77-137`
HeatmapGenerator / JointsGenerator; `:140-164` collate_fn).  The split:
  * host, numpy float64 (B * P * 17 points): the random draws -- from the same global RNGs in the reference's order, so that equal
    seeds give equal augmentations --, the affine matrices, the transformed / flipped joints and their integer form;
  * device: the image warp + flip + normalisation (hh_train_images_u8_batch), the crowd masks of all stages
    (hh_train_masks_u8_batch) and the target heatmaps (hh_render_heatmaps, one launch per stage).
Raw pixels, masks and descriptors cross in ONE host->device copy from a pinned, double-buffered staging area.  The result is what
`KeypointsModule.training_step` / `AEKeypointsLoss.calculate_loss` take: (images, [heatmaps], [masks], [DeviceJoints]).
There is no CPU path.  The warp is the project's restatement of cv2.warpAffine (parity with cv2 itself UNPINNED, as for
hh_preprocess_u8).

The mosaic of the reference's dataset (`mosaic_probability`, src/keypoints/config.py:44; coco.py:459-462 and :300-370
get_raw_mosaiced_data) is part of it: a `Mosaic` entry of the batch ships its four raw tiles in the same copy, ONE
hh_mosaic_u8_batch launch resizes them into a 2S x 2S image canvas and mask canvas behind the staged bytes on the device (S =
out_size), and the two warp launches read those canvases like any raw sample.  The joints of the four tiles are shifted and scaled
on the host (`mosaic_joints`).  The resize is the project's restatement of cv2.resize's 8-bit INTER_LINEAR (include/hhrnet.h;
parity with cv2 itself UNPINNED as well).
"""
from __future__ import annotations

import ctypes as C
import random
from dataclasses import dataclass

import numpy as np

from .. import _lib
from .._stage import Layout, PinnedRing, align
from . import crowd_mask as cm
from . import jpeg as jp
from .loss import DeviceJoints, pack_joints
from .targets import JointsGenerator
from .transforms_utils import COCO_FLIP_INDEX

MAX_STAGES = _lib.const("TRAIN_MAX_STAGES")
_TRAIN_DESC, _MOSAIC_DESC = _lib.struct_dtype("hh_train_desc"), _lib.struct_dtype("hh_mosaic_desc")


@dataclass
class AugParams:
    """One sample's augmentation: `scale` is the reference's `scale` after `*= aug_scale` (units of 200 px), `rot` in degrees,
    `center` in raw-image pixels after the translation."""
    scale: float
    rot: float
    center: tuple
    flip: bool


def _hw(img) -> tuple:
    """(h, w) of a sample's image: a pixel array, or a jpeg.JpegImage (which carries the size of what it decodes to)."""
    return tuple(img.shape[:2]) if isinstance(img, jp.JpegImage) else np.asarray(img).shape[:2]


class Mosaic:
    """A batch entry of `TrainInput.build` that stands where a raw sample may stand: four raw samples (image, mask, joints) that are
    resized to out_size x out_size each and tiled top-left, top-right, bottom-left, bottom-right (coco.py:318-325)."""

    def __init__(self, tiles):
        self.tiles = list(tiles)
        if len(self.tiles) != 4:
            raise ValueError("Mosaic: exactly four raw samples")


def mosaic_joints(tiles, S: int, num_kpts: int = 17) -> np.ndarray:
    """The joints of get_raw_mosaiced_data (coco.py:330-342) followed by get_coco_joints (:68-74): per tile x * (S / w) + s_x,
    y * (S / h) + s_y, rows with vis <= 0 zeroed, the four tiles' people concatenated in tile order -> float64 [P_total,K,3].  The
    assignment is numpy's, as in the reference: joints given as an INTEGER array (COCO's annotations) are truncated toward zero,
    joints given as a float array are not.  The tiles' arrays are not modified."""
    out = [np.zeros((0, num_kpts, 3))]
    for i, (img, _, joints) in enumerate(tiles):
        h, w = _hw(img)
        k = np.array(joints).reshape(-1, num_kpts, 3)  # a copy that keeps the dtype
        hidden = k[:, :, 2] <= 0
        k[:, :, 0] = k[:, :, 0] * (S / w) + (i % 2) * S
        k[:, :, 1] = k[:, :, 1] * (S / h) + (i // 2) * S
        k[hidden] = k[hidden] * 0
        out.append(k.astype(np.float64))
    return np.concatenate(out)


def affine_matrix(center, scale: float, res, rot: float = 0) -> np.ndarray:
    """RandomAffineTransform._get_affine_matrix (transforms.py:95-119) -> 3x3 float64: raw pixels -> a res = (h, w) map that shows the
    200 * scale px square around `center`, rotated by -rot degrees about the map's centre."""
    side = 200 * scale
    t = np.zeros((3, 3))
    t[0, 0], t[1, 1], t[2, 2] = float(res[1]) / side, float(res[0]) / side, 1
    t[0, 2] = res[1] * (-float(center[0]) / side + 0.5)
    t[1, 2] = res[0] * (-float(center[1]) / side + 0.5)
    if not rot == 0:
        rad = -rot * np.pi / 180
        sn, cs = np.sin(rad), np.cos(rad)
        turn = np.array([[cs, -sn, 0], [sn, cs, 0], [0, 0, 1]])
        to_origin = np.eye(3)
        to_origin[0, 2], to_origin[1, 2] = -res[1] / 2, -res[0] / 2
        back = to_origin.copy()
        back[:2, 2] *= -1
        t = np.dot(back, np.dot(turn, np.dot(to_origin, t)))
    return t


def affine_joints(xy: np.ndarray, mat: np.ndarray) -> np.ndarray:
    """RandomAffineTransform._affine_joints (transforms.py:121-127): (x, y, 1) @ mat.T for every point."""
    xy = np.array(xy, np.float64)
    pts = xy.reshape(-1, 2)
    return np.dot(np.concatenate((pts, pts[:, 0:1] * 0 + 1), axis=1), mat.T).reshape(xy.shape)


def bump_table(sigma: float) -> tuple[np.ndarray, int]:
    """The reference's `gauss` (coco.py:89-92) cast to fp32, and its reach 3 sigma + 1.  Sigmas the render kernel does not take
    (3 sigma + 1 not an integer, more than 63 entries a side) raise HHError with hh_heatmap_table_size's message."""
    n, reach = C.c_int(), C.c_int()
    _lib.check(_lib.load().hh_heatmap_table_size(float(sigma), C.byref(n), C.byref(reach)))
    grid = np.arange(0, 6 * sigma + 3, 1, float)
    centre = 3 * sigma + 1
    table = np.exp(-((grid[None, :] - centre) ** 2 + (grid[:, None] - centre) ** 2) / (2 * sigma ** 2)).astype(np.float32)
    assert table.shape == (n.value, n.value)
    return np.ascontiguousarray(table), reach.value


class _Mode:
    """One of the two pipelines of the reference's KeypointsTransform (`.train` / `.inference`, transforms.py:190-220): the ranges
    its RandomAffineTransform draws from, and whether a flip is drawn."""

    def __init__(self, owner: "TrainInput", max_rotation, min_scale, max_scale, max_translate, flip_p):
        self.owner = owner
        self.max_rotation, self.min_scale, self.max_scale, self.max_translate, self.flip_p = max_rotation, min_scale, max_scale, max_translate, flip_p

    def draw(self, height: int, width: int) -> AugParams:
        """transforms.py:137-153 then :65: np.random.random() for the scale, np.random.random() for the rotation, np.random.randint
        twice when max_translate > 0, random.random() for the flip (train only)."""
        center = np.array((width / 2, height / 2))
        scale = (max if self.owner.scale_type == "long" else min)(height, width) / 200
        scale *= np.random.random() * (self.max_scale - self.min_scale) + self.min_scale
        rot = (np.random.random() * 2 - 1) * self.max_rotation
        if self.max_translate > 0:
            reach = int(self.max_translate * scale)
            center[0] += np.random.randint(-reach, reach)
            center[1] += np.random.randint(-reach, reach)
        flip = self.flip_p is not None and random.random() < self.flip_p
        return AugParams(float(scale), float(rot), (float(center[0]), float(center[1])), bool(flip))

    def choose(self, samples, pool=None):
        """The per-item draws of the reference's dataset and transform in its order (coco.py:459, :305, then `draw`): with
        mosaic_probability > 0 one random.random() per sample, for a mosaic three random.randint(0, len(pool) - 1) (the sample
        itself is tile 0, repeats are allowed) and the augmentation of a 2S x 2S image.  -> (entries for `build`, [AugParams]).
        With mosaic_probability == 0 no extra draw is made (the reference draws random.random() even then: a stated deviation that
        keeps the draws of the existing path)."""
        prob, S = self.owner.mosaic_probability, self.owner.out_size
        if prob > 0 and pool is None:
            raise ValueError("TrainInput: mosaic_probability > 0 needs a pool of raw samples: .train(samples, pool)")
        entries, params = [], []
        for s in samples:
            if prob > 0 and random.random() < prob:
                s = Mosaic([s] + [pool[random.randint(0, len(pool) - 1)] for _ in range(3)])
                params.append(self.draw(2 * S, 2 * S))
            else:
                params.append(self.draw(*_hw(s[0])))
            entries.append(s)
        return entries, params

    def __call__(self, samples, pool=None):
        return self.owner.build(*self.choose(samples, pool))


class TrainInput:
    """The reference's `KeypointsTransform(out_size, hm_resolutions, ...)` (transforms.py:175-220) together with the target
    generators of its dataset (`num_kpts`, `sigma`: coco.py:185-219), on batches.

        ti = TrainInput(512, [1 / 4, 1 / 2])
        batch = ti.train(samples)        # samples: [(uint8 HWC image, bool HW crowd mask, float [P,K,3] joints), ...]
        module.training_step(batch)

    `.train(samples)` / `.inference(samples)` draw the augmentation per sample (inference: no rotation / scale / translate /
    flip) and call `build(samples, params)`, the explicit-parameter entry.

    `mosaic_probability` is the field of the reference's dataset (both modes honour it: the dataset decides, not the transform).
    With a value > 0 a mode is called as `ti.train(samples, pool)`: `pool` is any object with len() and [i] -> (image, mask, joints)
    raw samples (the reference's get_raw_data), from which the three other tiles of a mosaic are drawn.  `build` takes a
    `Mosaic(tiles)` wherever it takes a raw sample.

    The image of a sample or of a mosaic tile may be a `jpeg.JpegImage` (the file's compressed bytes) instead of a pixel array: its
    pixels are decoded on the device and never cross the bus.  `jpeg_status()` reads the decoder's per-image statuses of the last
    build."""

    def __init__(self, out_size: int, hm_resolutions, max_rotation: int = 30, min_scale: float = 0.75, max_scale: float = 1.5,
                 scale_type: str = "short", max_translate: int = 40, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225),
                 num_kpts: int = 17, sigma: float = 2, flip_index=COCO_FLIP_INDEX, device="cuda:0", mosaic_probability: float = 0.0):
        assert scale_type in ("short", "long"), f"unknown scale type: {scale_type}"
        self.out_size, self.scale_type, self.num_kpts, self.device = int(out_size), scale_type, num_kpts, device
        self.mosaic_probability = float(mosaic_probability)
        self.hm_sizes = [int(r * out_size) for r in hm_resolutions]
        if not 0 < len(self.hm_sizes) <= MAX_STAGES:
            raise _lib.HHError(f"TrainInput: 1..{MAX_STAGES} heatmap stages, got {len(self.hm_sizes)}")
        self.mean, self.std = np.asarray(mean, np.float32), np.asarray(std, np.float32)
        self.flip_index = list(flip_index)
        self.sigmas = [s / 64 if sigma < 0 else sigma for s in self.hm_sizes]
        self.tables = [bump_table(s) for s in self.sigmas]  # refuses a sigma the kernel does not take, before any GPU work
        self.joints_generators = [JointsGenerator(s) for s in self.hm_sizes]
        self.train = _Mode(self, max_rotation, min_scale, max_scale, max_translate, 0.5)
        self.inference = _Mode(self, 0, 1, 1, 0, None)
        self._tables_dev = None
        self._ring = PinnedRing()  # pinned staging buffers, each with the event behind the copy that last read it
        self.last_h2d_bytes = self.last_launches = 0  # of the last build(): what tools/train_input_time.py reports
        self.last_staged_bytes = 0  # the part of last_h2d_bytes that is the one staged copy (the rest: the joint tables)
        self._jpeg_status = None    # the device statuses of the last build's JpegImage samples

    # ------------------------------------------------------------------ host half (no GPU)
    def geometry(self, height: int, width: int, joints, p: AugParams):
        """-> (image matrix 2x3, [stage matrix 2x3], [float joints [P,K,3] per stage], [int32 joints [P',K,3] per stage]): the matrices
        of transforms.py:155-170, the joints after the affine (:165) and the flip (:69-70), and after JointsGenerator."""
        joints = np.asarray(joints, np.float64).reshape(-1, self.num_kpts, 3)
        mat_image = affine_matrix(p.center, p.scale, (self.out_size, self.out_size), p.rot)[:2]
        mats, floats, ints = [], [], []
        for size, gen in zip(self.hm_sizes, self.joints_generators):
            mat = affine_matrix(p.center, p.scale, (size, size), p.rot)[:2]
            j = joints.copy()
            j[:, :, 0:2] = affine_joints(j[:, :, 0:2], mat)
            if p.flip:
                j = j[:, self.flip_index]
                j[:, :, 0] = size - j[:, :, 0] - 1
            mats.append(mat)
            floats.append(j)
            ints.append(gen(j))
        return mat_image, mats, floats, ints

    # ------------------------------------------------------------------ device half
    def build(self, samples, params):
        """samples: [(uint8 [h,w,3] image, bool [h,w] crowd mask, float [P,K,3] joints) or Mosaic of four of them], params: [AugParams]
        (of a 2S x 2S image for a Mosaic) -> (images [B,3,S,S], [heatmaps [B,K,s,s]], [masks [B,s,s]], [DeviceJoints]) on the device,
        in the current stream.  The crowd mask of a sample or tile may be a `crowd_mask.CrowdSegments` of the image's size instead
        of a dense array (`crowd_mask.raw_sample` makes such samples from COCO annotations); dense and segment samples may be mixed.
        A segment sample's mask bytes are not staged: its toggles and descriptors travel in the same copy, and one
        hh_crowd_masks_u8_batch launch per batch fills the masks behind the staged bytes of the device buffer, before the mosaic and
        warp launches.  A batch of dense samples takes exactly the path it took before: same bytes, same launches.
        The image of a sample or tile may be a `jpeg.JpegImage`, mixed freely with arrays: its stream and table block travel in the same
        copy (behind the crowd tables), its h * w * 3 pixel slot lies behind the staged bytes of the device buffer, and ONE
        hh_jpeg_decode_u8_batch call (three launches) fills all such slots before the crowd-mask, mosaic and warp launches.  Nothing
        synchronises here: `jpeg_status()` reads the statuses afterwards.  A batch without a JpegImage takes exactly the path it took
        before: same bytes, same launches."""
        import torch
        lib = _lib.load()
        B, S, K, nst = len(samples), self.out_size, self.num_kpts, len(self.hm_sizes)
        if B == 0 or len(params) != B:
            raise ValueError("TrainInput.build: one AugParams per sample, at least one sample")
        dp = C.POINTER(C.c_double)
        invert = lambda m: self._invert(lib, m, dp)  # noqa: E731

        # what travels: every raw sample once, a Mosaic's four tiles in its place (images first, then masks, as before)
        raws, slots = [], []  # slots[b]: index into raws, or the four indices of a Mosaic's tiles
        for entry in samples:
            tiles = entry.tiles if isinstance(entry, Mosaic) else [entry]
            for img, mask, _ in tiles:
                if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3 or mask.shape != img.shape[:2]:
                    raise ValueError("TrainInput.build: uint8 [h,w,3] images with [h,w] crowd masks only")
                if isinstance(img, jp.JpegImage) and img.device_index:
                    raise ValueError("TrainInput.build: a device-indexed JpegImage (index='device') is refused: training files come back every "
                                     "epoch, so build their index once on the host (jpeg.JpegIndexCache)")
            first = len(raws)
            raws.extend(tiles)
            slots.append(list(range(first, first + 4)) if isinstance(entry, Mosaic) else first)
        R, M = len(raws), sum(isinstance(e, Mosaic) for e in samples)
        shapes = [img.shape[:2] for img, _, _ in raws]
        # a raw sample whose second element is a CrowdSegments ships no mask bytes: its toggles and descriptors travel instead
        seg_raws = [r for r, (_, mask, _) in enumerate(raws) if isinstance(mask, cm.CrowdSegments)]
        seg_items = [raws[r][1] for r in seg_raws]
        jpeg_raws = [r for r, (img, _, _) in enumerate(raws) if isinstance(img, jp.JpegImage)]
        jpeg_items = [raws[r][0] for r in jpeg_raws]
        sizes = [0 if isinstance(img, jp.JpegImage) else h * w * 3 for (h, w), (img, _, _) in zip(shapes, raws)] + [0 if isinstance(mask, cm.CrowdSegments) else h * w for (h, w), (_, mask, _) in zip(shapes, raws)]
        offs = np.cumsum([0] + sizes)
        desc_off = align(int(offs[-1]))  # the descriptors travel behind the pixels and masks, in the same copy
        mosaic_off = desc_off + _TRAIN_DESC.itemsize * B
        crowd_off = mosaic_off + _MOSAIC_DESC.itemsize * M  # (a multiple of 8: both descriptor sizes are)
        lay = Layout(crowd_off + cm.tables_bytes(seg_items))
        # a JpegImage ships its stream and table block behind the crowd tables: [decode descriptors | stream, tables | ...], 16-aligned
        jpegs = jp.JpegBatch(jpeg_items, what="TrainInput.build")
        jpegs.place_upload(lay)
        total = lay.end
        # the canvases of the mosaic samples lie behind the staged bytes in the device buffer; nothing of them is copied
        canvas_off = align(total)
        # ... and behind them the masks of the segment samples, which hh_crowd_masks_u8_batch fills there
        fill_offs = canvas_off + M * 16 * S * S + np.cumsum([0] + [(s.h * s.w + 3) // 4 * 4 for s in seg_items])
        mask_at_raw = [int(offs[R + r]) for r in range(R)]
        for i, r in enumerate(seg_raws):
            mask_at_raw[r] = int(fill_offs[i])
        # ... and behind those the statuses and the pixel slots of the JpegImage samples, which hh_jpeg_decode_u8_batch fills there
        lay.end = int(fill_offs[-1])
        jpegs.place_device(lay)
        device_bytes = lay.end
        image_at_raw = [int(offs[r]) for r in range(R)]
        for r, at in zip(jpeg_raws, jpegs.pixel_at):
            image_at_raw[r] = at
        if M and (S % 4 or S < 4):
            raise _lib.HHError("TrainInput.build: a mosaic needs an out_size that is a multiple of 4 (hh_mosaic_u8_batch)")
        turn, host = self._ring.take(total)
        hview = host.numpy()
        descs = hview[desc_off:mosaic_off].view(_TRAIN_DESC)
        mdescs = hview[mosaic_off:crowd_off].view(_MOSAIC_DESC)
        crowd_desc_at, crowd_seg_at, crowd_nseg = cm.fill_tables(seg_items, fill_offs[:-1], hview, crowd_off)
        jpegs.fill(hview)
        for r, (img, mask, _) in enumerate(raws):
            h, w = shapes[r]
            if not isinstance(img, jp.JpegImage):
                np.copyto(hview[offs[r]:offs[r + 1]].reshape(h, w, 3), img)
            if isinstance(mask, cm.CrowdSegments):
                continue
            mview = hview[offs[R + r]:offs[R + r + 1]].reshape(h, w)
            np.multiply(mask, 255, out=mview, casting="unsafe")  # (mask * 255).astype(np.uint8), transforms.py:159
        stage_joints = [[] for _ in range(nst)]
        m = 0
        for b, (entry, p) in enumerate(zip(samples, params)):
            if isinstance(entry, Mosaic):
                image_at, mask_at = canvas_off + m * 16 * S * S, canvas_off + m * 16 * S * S + 12 * S * S
                mdescs[m] = ([(image_at_raw[r], mask_at_raw[r], *shapes[r]) for r in slots[b]], image_at, mask_at)
                h = w = 2 * S
                joints = mosaic_joints(entry.tiles, S, K)
                m += 1
            else:
                image_at, mask_at, (h, w), joints = image_at_raw[slots[b]], mask_at_raw[slots[b]], shapes[slots[b]], entry[2]
            mat_image, mats, _, ints = self.geometry(h, w, joints, p)
            inv_mask = np.zeros((MAX_STAGES, 6))
            for i, mat in enumerate(mats):
                inv_mask[i] = invert(mat)
                stage_joints[i].append(ints[i])
            descs[b] = (image_at, mask_at, h, w, int(p.flip), 0, invert(mat_image), inv_mask)

        dev = torch.device(self.device)
        with torch.cuda.device(dev):
            cur = torch.cuda.current_stream(dev)
            if M or seg_items or jpeg_items:
                raw = torch.empty(device_bytes, device=dev, dtype=torch.uint8)
                raw[:total].copy_(host[:total], non_blocking=True)
            else:
                raw = host[:total].to(dev, non_blocking=True)
            copied = torch.cuda.Event()
            copied.record(cur)
            self._ring.release(turn, copied)
            self.last_h2d_bytes, self.last_launches = total, 2 + nst + (1 if M else 0) + (1 if seg_items else 0) + (3 if jpeg_items else 0)
            self.last_staged_bytes = total
            if self._tables_dev is None:
                self._tables_dev = [torch.from_numpy(t).to(dev) for t, _ in self.tables]
            images = torch.empty((B, 3, S, S), device=dev, dtype=torch.float32)
            masks = [torch.empty((B, s, s), device=dev, dtype=torch.float32) for s in self.hm_sizes]
            heatmaps = [torch.empty((B, K, s, s), device=dev, dtype=torch.float32) for s in self.hm_sizes]
            base = raw.data_ptr()
            self._jpeg_status = jpegs.launch(raw)  # the pixels of the JpegImage samples first of all: everything below reads them
            if seg_items:  # the masks of the segment samples first: the mosaic and the mask warp read them
                cm.launch(dev, base, host.data_ptr(), crowd_desc_at, crowd_seg_at, len(seg_items), crowd_nseg)
            if M:  # the canvases next: the two warp launches below read them
                _lib.launch(dev, lib.hh_mosaic_u8_batch, base, base + mosaic_off, mdescs.ctypes.data, M, S)
            _lib.launch(dev, lib.hh_train_images_u8_batch, base, base + desc_off, B, images.data_ptr(), S, S, self.mean.ctypes.data,
                        self.std.ctypes.data)
            stage_hw = (C.c_int * (2 * nst))(*[s for s in self.hm_sizes for _ in range(2)])
            outs = (C.c_void_p * nst)(*[m.data_ptr() for m in masks])
            _lib.launch(dev, lib.hh_train_masks_u8_batch, base, base + desc_off, B, nst, stage_hw, outs)
            device_joints = []
            for i, s in enumerate(self.hm_sizes):
                packed, counts = pack_joints(stage_joints[i], K, s, s)
                self.last_h2d_bytes += packed.nbytes + counts.nbytes
                dj = DeviceJoints(torch.from_numpy(packed).to(dev), torch.from_numpy(counts).to(dev), (K, s, s))
                table, reach = self._tables_dev[i], self.tables[i][1]
                _lib.launch(dev, lib.hh_render_heatmaps, dj.packed.data_ptr(), dj.counts.data_ptr(), B, packed.shape[1], K, table.data_ptr(),
                            table.shape[0], reach, heatmaps[i].data_ptr(), s, s)
                device_joints.append(dj)
        return images, heatmaps, masks, device_joints

    def plot_examples(self, annotated, params=None, names=None, nrows: int = 1, stage_idxs=(1, 0), labels=None, device_out: bool = False):
        """The figure the reference's DatasetExamplesCallback logs (CocoKeypointsDataset.plot_examples, coco.py:372-449), from a batch
        built here.  annotated: [(image or jpeg.JpegImage, COCO annotation list)], or (image, annot, dense bool crowd mask) to ship that
        mask instead of the annotation's segments.  Raw samples are made with crowd_mask.raw_sample, `params` are drawn with
        `self.train.choose` when none are given, `build` makes the batch, `geometry` gives the per-stage integer joints, and
        keypoints/sample_plot.py composes the figure on the device.  `names`: the file stems shown in the labels.
        Mosaic samples are not plotted (a mosaic has no single raw image for the raw pane): with `mosaic_probability > 0` every
        sample is shown as a plain sample and its augmentation is drawn with `self.train.draw`, without the mosaic's draws.
        -> uint8 [H,W,3] numpy array, or the device tensor with `device_out` (for jpeg.encode_jpeg_device / save_jpeg)."""
        from . import sample_plot as sp
        from .visualization import to_host
        raws = []
        for entry in annotated:
            h, w = _hw(entry[0])
            _, segments, joints = cm.raw_sample(np.empty((h, w, 0), np.uint8), entry[1], self.num_kpts)  # (only the size is read)
            raws.append((entry[0], entry[2] if len(entry) > 2 else segments, joints))
        if params is None:  # (choose makes no draw besides the samples' own when mosaic_probability == 0)
            params = self.train.choose(raws)[1] if self.mosaic_probability == 0 else [self.train.draw(*_hw(r[0])) for r in raws]
        images, heatmaps, masks, _ = self.build(raws, params)
        items = []
        for b, (entry, raw, p) in enumerate(zip(annotated, raws, params)):
            ints = self.geometry(*_hw(raw[0]), raw[2], p)[3]
            sample = (images[b], [hm[b] for hm in heatmaps], [m[b] for m in masks], ints)
            items.append((entry[0], entry[1], sample, str(names[b]) if names is not None else f"{b:012d}"))
        figure = sp.plot_examples_device(items, nrows, stage_idxs, sp.COCO_LABELS if labels is None else labels)
        return figure if device_out else to_host(figure)

    def jpeg_status(self, check: bool = True) -> np.ndarray:
        """The decoder's statuses of the last build's JpegImage samples, in batch order (tiles of a mosaic in tile order): int32 [n], 0 =
        decoded.  This is the read `build` does not do: it waits for the build's work.  `check`: a nonzero status raises HHError naming
        the image and the code.  (A sample whose index the host built was validated there already.)"""
        if self._jpeg_status is None:
            return np.zeros(0, np.int32)
        status = self._jpeg_status.cpu().numpy()
        if check:
            jp.raise_status(status, "TrainInput.build (hh_jpeg_decode_u8_batch)")
        return status

    @staticmethod
    def _invert(lib, m, dp) -> np.ndarray:
        fwd = np.ascontiguousarray(np.asarray(m, np.float64).reshape(6))
        inv = np.empty(6, np.float64)
        _lib.check(lib.hh_invert_affine(fwd.ctypes.data_as(dp), inv.ctypes.data_as(dp)))
        return inv
