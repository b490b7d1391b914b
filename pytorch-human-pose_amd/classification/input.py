"""The classifier's input built on the device: random / centre crops of raw uint8 images, antialiased resize, flip, normalisation.

Stands in for what the reference's dataset worker does per image on the host with torchvision
(`src/classification/transforms.py:14-30` ClassificationTransform: `.train` = ToTensor -> RandomResizedCrop(224, antialias=True) ->
RandomHorizontalFlip -> Normalize, `.inference` = ToTensor -> Resize(int(224 / 0.875), antialias=True) -> CenterCrop(224) ->
Normalize) and for the transform of `src/classification/model.py:45-57`.  The split:
  * host: the random draws (torch's global RNG, torchvision's published procedure) and the Resize / CenterCrop geometry: ten integers
    per sample;
  * device: crop, separable triangle-filter resample (torch's upsample_bilinear2d_aa, align_corners=False), window, flip, ToTensor
    and Normalize in ONE launch per batch (hh_resized_crop_u8_batch, csrc/cls_input.hip).
The raw pixels of every sample's source rectangle (the crop; not the image around it), the descriptors and the targets cross in ONE
host->device copy from a pinned, double-buffered staging area.  The result is what `ClassificationModule.training_step` /
`validation_step` take: (images [B,3,S,S] fp32, targets int64), on the device.
There is no CPU path.
A sample's image may also be a `keypoints.jpeg.JpegImage`, the file's compressed bytes: its crop rectangle is then the window of ONE
hh_jpeg_decode_window_u8_batch call per batch (three launches in front of the one above), and only the byte slice and the table block
that window needs cross, in the same copy (`ClsInput.build`).  The result is bit-identical to the batch built from the decoded arrays.

UNPINNED: torchvision is not installed where this project is built and tested, so (a) the ORDER and kind of the random draws of
`random_resized_crop_params` follow torchvision's published `RandomResizedCrop.get_params` / `RandomHorizontalFlip.forward` but
have not been compared with a torchvision run under equal seeds, and (b) whether `T.Resize(size)` without an `antialias` argument
antialiases a tensor depends on the torchvision version (it did not before 0.17), which is why the flag travels in the descriptor
and `InferenceClassificationModel` takes it as an argument.  The deterministic part -- `build` from explicit parameters -- is pinned
against torch's own F.interpolate and a float64 restatement (tests/cls_input_budget.py).
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

from .. import _lib
from .._stage import Layout, PinnedRing, align
from ..keypoints import jpeg as jp
from ..keypoints.transforms_utils import IMAGENET_MEAN, IMAGENET_STD

# hh_crop_desc of include/hhrnet.h (56 bytes)
_CROP_DESC = _lib.struct_dtype("hh_crop_desc")


def _hw(img) -> tuple:
    """(h, w) of a sample's image: a pixel array, or a jpeg.JpegImage (which carries the size of what it decodes to)."""
    return tuple(img.shape[:2]) if isinstance(img, jp.JpegImage) else np.asarray(img).shape[:2]


@dataclass
class CropParams:
    """One sample's augmentation: the crop rectangle in raw-image pixels (it is resized to the whole output) and the flip."""
    top: int
    left: int
    height: int
    width: int
    flip: bool = False


@dataclass
class CropWindow:
    """The general form of one sample (every field of hh_crop_desc but the image's own): the source rectangle, the size of the
    virtual resized crop, the origin of the output window inside it, flip and antialias."""
    top: int
    left: int
    height: int
    width: int
    rh: int
    rw: int
    oy: int = 0
    ox: int = 0
    flip: bool = False
    antialias: bool = True


def random_resized_crop_params(height: int, width: int, scale=(0.08, 1.0), ratio=(3 / 4, 4 / 3), flip_p: float | None = 0.5) -> CropParams:
    """torchvision's RandomResizedCrop.get_params then RandomHorizontalFlip, from torch's global RNG: up to 10 attempts, each drawing
    the area uniformly in `scale` (of the image's area) and the aspect ratio log-uniformly in `ratio`, rounding to an integer size and,
    if that fits the image, drawing the offsets with randint; if none fits, the central crop with the image's ratio clamped to
    `ratio`.  The flip is `torch.rand(1) < flip_p`, drawn after the crop (flip_p None: no draw).  Draw order UNPINNED against a
    torchvision run (see the module docstring)."""
    import torch
    area = height * width
    log_lo, log_hi = math.log(ratio[0]), math.log(ratio[1])
    rect = None
    for _ in range(10):
        target_area = area * torch.empty(1).uniform_(scale[0], scale[1]).item()
        aspect = math.exp(torch.empty(1).uniform_(log_lo, log_hi).item())
        w = int(round(math.sqrt(target_area * aspect)))
        h = int(round(math.sqrt(target_area / aspect)))
        if 0 < w <= width and 0 < h <= height:
            top = int(torch.randint(0, height - h + 1, size=(1,)).item())
            left = int(torch.randint(0, width - w + 1, size=(1,)).item())
            rect = (top, left, h, w)
            break
    if rect is None:
        rect = central_crop_fallback(height, width, ratio)
    flip = flip_p is not None and bool(torch.rand(1).item() < flip_p)
    return CropParams(*rect, flip)


def central_crop_fallback(height: int, width: int, ratio=(3 / 4, 4 / 3)) -> tuple:
    """The crop RandomResizedCrop falls back to: the whole image where its width / height lies within `ratio`, else the central part
    with the ratio clamped -> (top, left, h, w)."""
    in_ratio = float(width) / float(height)
    if in_ratio < min(ratio):
        w = width
        h = int(round(w / min(ratio)))
    elif in_ratio > max(ratio):
        h = height
        w = int(round(h * max(ratio)))
    else:
        w, h = width, height
    return (height - h) // 2, (width - w) // 2, h, w


def inference_geometry(height: int, width: int, resize: int = 256, crop: int = 224) -> tuple:
    """Resize(resize) + CenterCrop(crop) of an image of height x width -> (rh, rw, oy, ox): the short side goes to `resize`, the long
    side to int(resize * long / short); the crop x crop window starts at int(round((r - crop) / 2.0)) on each axis."""
    short, long = (width, height) if width <= height else (height, width)
    new_short, new_long = resize, int(resize * long / short)
    rw, rh = (new_short, new_long) if width <= height else (new_long, new_short)
    return rh, rw, int(round((rh - crop) / 2.0)), int(round((rw - crop) / 2.0))


class ClsInput:
    """The reference's `ClassificationTransform(out_size, mean, std)` (classification/transforms.py:6-31) on batches.

        ci = ClsInput(224)
        batch = ci.train(samples)          # samples: [(uint8 HWC image, int target), ...]
        module.training_step(batch)

    `.train(samples)` draws a RandomResizedCrop + flip per sample, `.inference(samples)` takes Resize(int(out_size / resize_ratio)) +
    CenterCrop(out_size); both call `build(samples, params)`, the explicit entry, whose params are per sample a CropParams, an
    `inference_geometry` tuple (rh, rw, oy, ox) or a CropWindow."""

    def __init__(self, out_size: int = 224, mean=IMAGENET_MEAN, std=IMAGENET_STD, resize_ratio: float = 0.875, device="cuda:0",
                 antialias: bool = True):
        self.out_size, self.device, self.antialias = int(out_size), device, bool(antialias)
        self.resize = int(out_size / resize_ratio)  # transforms.py:26
        self.mean, self.std = np.asarray(mean, np.float32), np.asarray(std, np.float32)
        self._ring = PinnedRing()  # pinned staging buffers, each with the event behind the copy that last read it
        self.last_h2d_bytes = self.last_launches = 0  # of the last build(): what tools/cls_input_time.py reports
        self._jpeg_status = None  # the device statuses of the last build's JpegImage samples

    def train(self, samples):
        return self.build(samples, [random_resized_crop_params(*_hw(s[0])) for s in samples])

    def inference(self, samples):
        return self.build(samples, [inference_geometry(*_hw(s[0]), resize=self.resize, crop=self.out_size) for s in samples])

    def window(self, height: int, width: int, p) -> CropWindow:
        """One sample's parameters in the general form."""
        S = self.out_size
        if isinstance(p, CropWindow):
            return p
        if isinstance(p, CropParams):  # the crop becomes the whole output
            return CropWindow(p.top, p.left, p.height, p.width, S, S, 0, 0, p.flip, self.antialias)
        rh, rw, oy, ox = p             # the whole image resized, a window of it
        return CropWindow(0, 0, height, width, rh, rw, oy, ox, False, self.antialias)

    @staticmethod
    def layout(shapes) -> tuple:
        """Byte layout of the one buffer that crosses, from the (height, width) of every sample's source rectangle (only the crop is
        shipped, not the image around it): the pixels back to back, then (64-byte aligned) the descriptors, then the int64
        targets -> (image offsets, descriptor offset, target offset, total)."""
        offs = np.cumsum([0] + [h * w * 3 for h, w in shapes])
        desc_off = align(int(offs[-1]))
        target_off = desc_off + _CROP_DESC.itemsize * len(shapes)  # 56 B descriptors: a multiple of 8
        return offs, desc_off, target_off, target_off + 8 * len(shapes)

    def build(self, samples, params):
        """samples: [(uint8 [h,w,3] image, int target)], params: one CropParams / (rh, rw, oy, ox) / CropWindow per sample ->
        (images [B,3,S,S] fp32, targets [B] int64) on the device, in the current stream.
        A sample's image may be a `jpeg.JpegImage` (the file's compressed bytes), mixed freely with arrays: its source rectangle is its
        decode window.  The slice of the stream that the window's segments need and their table block travel in the same copy, behind
        the targets; its height x width x 3 pixel slot lies behind the staged bytes of the device buffer, and ONE
        hh_jpeg_decode_window_u8_batch call (three launches) fills all such slots before the resized-crop launch, which reads a slot
        exactly as it reads a shipped crop.  Nothing synchronises here: `jpeg_status()` reads the statuses afterwards.  A stream the
        decoder does not take (progressive, CMYK, ...) is refused by name at `JpegImage(...)`: pass such a file as a Pillow array in
        the same batch; there is no silent fallback.  A batch without a JpegImage takes exactly the path it took before."""
        import torch
        lib = _lib.load()
        B, S = len(samples), self.out_size
        if B == 0 or len(params) != B:
            raise ValueError("ClsInput.build: one parameter set per sample, at least one sample")
        windows = []
        for b, ((img, _), p) in enumerate(zip(samples, params)):
            if not isinstance(img, jp.JpegImage) and (not isinstance(img, np.ndarray) or img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3):
                raise ValueError("ClsInput.build: uint8 [h,w,3] images (or jpeg.JpegImage) only")
            if isinstance(img, jp.JpegImage) and img.device_index:
                raise ValueError("ClsInput.build: a device-indexed JpegImage (index='device') is refused: the crop's window needs the offsets on "
                                 "the host, and training files come back every epoch (jpeg.JpegIndexCache)")
            q = self.window(img.shape[0], img.shape[1], p)
            # only the source rectangle is staged and shipped (a slice would silently clip a rectangle that leaves the image)
            if q.height <= 0 or q.width <= 0 or q.top < 0 or q.left < 0 or q.top + q.height > img.shape[0] or q.left + q.width > img.shape[1]:
                raise _lib.HHError(f"ClsInput.build: sample {b}: crop rectangle outside its image (or empty)")
            windows.append(q)
        shapes = [(q.height, q.width) for q in windows]
        jpeg_at = [b for b, (img, _) in enumerate(samples) if isinstance(img, jp.JpegImage)]
        # a JpegImage ships no pixels: its slot in the pixel area is empty
        offs, desc_off, target_off, total = self.layout([(0, 0) if isinstance(img, jp.JpegImage) else hw for hw, (img, _) in zip(shapes, samples)])
        image_at = [int(o) for o in offs[:-1]]
        # behind the targets, 16-aligned: [decode descriptors | slice, tables | ...]; behind the staged bytes, on the device only: the
        # decode's statuses and the pixel slots it fills
        jpegs = jp.JpegBatch([samples[b][0] for b in jpeg_at],
                             [samples[b][0].window_plan((windows[b].top, windows[b].left, *shapes[b])) for b in jpeg_at], "ClsInput.build")
        lay = Layout(total)
        jpegs.place_upload(lay)
        total = lay.end
        jpegs.place_device(lay)
        for b, at in zip(jpeg_at, jpegs.pixel_at):
            image_at[b] = at
        turn, host = self._ring.take(total)
        hview = host.numpy()
        descs = hview[desc_off:target_off].view(_CROP_DESC)
        targets_host = hview[target_off:target_off + 8 * B].view(np.int64)
        for b, ((img, target), q) in enumerate(zip(samples, windows)):
            h, w = shapes[b]
            if not isinstance(img, jp.JpegImage):
                np.copyto(hview[offs[b]:offs[b + 1]].reshape(h, w, 3), img[q.top:q.top + h, q.left:q.left + w])
            # the shipped image IS the crop: tap indices are relative to the crop and never leave it, so nothing else is read
            descs[b] = (image_at[b], h, w, 0, 0, h, w, q.rh, q.rw, q.oy, q.ox, int(bool(q.flip)), int(bool(q.antialias)))
            targets_host[b] = int(target)
        jpegs.fill(hview)

        dev = torch.device(self.device)
        with torch.cuda.device(dev):
            cur = torch.cuda.current_stream(dev)
            if jpeg_at:
                raw = torch.empty(lay.end, device=dev, dtype=torch.uint8)
                raw[:total].copy_(host[:total], non_blocking=True)
            else:
                raw = host[:total].to(dev, non_blocking=True)
            copied = torch.cuda.Event()
            copied.record(cur)
            self._ring.release(turn, copied)
            self.last_h2d_bytes, self.last_launches = total, 4 if jpeg_at else 1
            images = torch.empty((B, 3, S, S), device=dev, dtype=torch.float32)
            base = raw.data_ptr()
            self._jpeg_status = jpegs.launch(raw)  # the pixels of the JpegImage samples first: the launch below reads them
            # the descriptors are checked on their HOST copy in the staging buffer (nothing is read back from the device)
            _lib.launch(dev, lib.hh_resized_crop_u8_batch, base, base + desc_off, descs.ctypes.data, B, images.data_ptr(), S, S,
                        self.mean.ctypes.data, self.std.ctypes.data)
            targets = raw[target_off:target_off + 8 * B].view(torch.int64)
        return images, targets

    def jpeg_status(self, check: bool = True) -> np.ndarray:
        """The decoder's statuses of the last build's JpegImage samples, in batch order: int32 [n], 0 = decoded.  This is the read
        `build` does not do: it waits for the build's work.  `check`: a nonzero status raises HHError naming the image (its position
        among the JpegImage samples) and the code.  A status covers the walked part of the scan only; the index pass (or restart scan)
        of `JpegImage(...)` has validated the whole stream."""
        if self._jpeg_status is None:
            return np.zeros(0, np.int32)
        status = self._jpeg_status.cpu().numpy()
        if check:
            jp.raise_status(status, "ClsInput.build (hh_jpeg_decode_window_u8_batch)")
        return status
