"""The classifier's plot: `plot_top_preds` of the reference (classification/visualization.py) on the device text kernel
(keypoints/text.py, hh_text_labels_u8_batch).  The host picks the font scale, orders the top-k and lays both boxes out; the pixels
are drawn on the GPU.  There is no CPU fallback."""
from __future__ import annotations

import numpy as np
import torch

from .. import _lib
from .._stage import Block, Layout, fill_frames, frames_to_host
from ..keypoints import text as tx
from ..keypoints import visualization as vz

TARGET_COLOR = (80, 255, 80)


def font_scale_for(img_h: int, img_w: int) -> float:
    """visualization.py:13-19: 0.3 up to a shorter side of 224, 0.5 up to 336, 0.7 beyond."""
    min_size = min(img_h, img_w)
    return 0.3 if 0 < min_size <= 224 else 0.5 if 224 < min_size <= 336 else 0.7


def top_preds_labels(probs: np.ndarray, idx2label: dict, k: int = 5) -> list[str]:
    """visualization.py:20-22: the k largest, the largest first, in np.argsort's order reversed (of equal values the higher index first)."""
    return [f"{probs[idx]:.3f}:  {idx2label[idx]}" for idx in reversed(np.argsort(probs)[-k:])]


def top_preds_table(img_h: int, img_w: int, probs: np.ndarray, idx2label: dict, k: int = 5, target_label=None, return_layout: bool = False):
    """The primitive table of plot_top_preds on an img_h x img_w image: the top-k box top-left and, with a target, the green
    "Target:" box bottom-right behind it, both at alpha 0.8.  `return_layout`: also [(labels, layout_put_txt's layout)] per box."""
    font_scale = font_scale_for(img_h, img_w)
    calls = [(top_preds_labels(probs, idx2label, k), dict(alpha=0.8, font_scale=font_scale, thickness=1))]
    if target_label is not None:
        calls.append((["Target:", str(target_label)], dict(loc="br", txt_color=TARGET_COLOR, alpha=0.8, font_scale=font_scale)))
    parts = [tx.layout_put_txt(img_h, img_w, labels, return_layout=True, **kw) for labels, kw in calls]
    table = np.concatenate([t for t, _ in parts])
    return (table, [(labels, lay) for (labels, _), (_, lay) in zip(calls, parts)]) if return_layout else table


def plot_top_preds(image, probs: np.ndarray, idx2label: dict, k: int = 5, target_label=None):
    """The reference's plot_top_preds, same signature -> a drawn copy: uint8 [h,w,3] numpy for a numpy image (uploaded, drawn, copied
    back), a device tensor for a device tensor.  Raises when the library or the GPU is missing."""
    table = top_preds_table(image.shape[0], image.shape[1], probs, idx2label, k, target_label)
    if isinstance(image, torch.Tensor):
        return tx.put_txt_device([image.clone(memory_format=torch.contiguous_format)], [table])[0]
    return frames_to_host(_plot_device([np.ascontiguousarray(image, dtype=np.uint8)], lambda frames: [table]))[0]


def _resize_512(frame: torch.Tensor) -> torch.Tensor:
    """resize_with_aspect_ratio(image, height=512, width=None) (utils/image.py:146-162): new_w = int(512 * w / h), cv2.resize."""
    h, w = int(frame.shape[0]), int(frame.shape[1])
    return frame if h == 512 else vz.resize_device(frame, int(512 * w / h), 512)


def _plot_device(images: list, tables_of, resize=None) -> list:
    """ONE upload of the host images (one pinned block), the resizes, ONE text launch -> drawn device frames.  `tables_of(frames)`
    gives one table per frame, for the sizes the frames have after the resize."""
    if not torch.cuda.is_available():
        raise _lib.HHError("plot_top_preds needs the GPU: there is no CPU renderer")
    device = torch.device("cuda", torch.cuda.current_device())
    if not all(im.dtype == np.uint8 and im.ndim == 3 and im.shape[2] == 3 for im in images):
        raise ValueError("plot_top_preds: a uint8 [h,w,3] image is needed")
    lay = Layout()
    places = [lay.add(im.size) for im in images]
    blk = Block(lay.pad(), lay.end, device)
    fill_frames(blk, images, places)
    blk.upload()
    frames = [blk.tensor(at, im.shape) for at, im in zip(places, images)]
    if resize is not None:
        frames = [resize(f) for f in frames]
    return tx.put_txt_device(frames, tables_of(frames))


def _inference_inputs(record):
    """results.py:70-74 of the reference: probs = exp(logits) / sum(exp(logits)) in the logits' own precision; the raw pixels."""
    e = np.exp(record.logits)
    raw = record.raw_image
    if not isinstance(raw, np.ndarray):  # a jpeg.JpegImage or a JPEG file's bytes: the host decoder, bit-identical to the device's
        from ..keypoints.jpeg import decode_jpeg_host
        raw = decode_jpeg_host(raw.data if hasattr(raw, "stage") else raw)
    return np.ascontiguousarray(raw, dtype=np.uint8), e / np.sum(e)


def plot_top_preds_device(records: list) -> list:
    """`InferenceClassificationResult.plot()` of every record on the device: every raw image resized to height 512 (hh_resize_u8),
    then one text launch for all -> device uint8 [512,w,3] frames."""
    inputs = [_inference_inputs(r) for r in records]

    def tables_of(frames):
        return [top_preds_table(int(f.shape[0]), int(f.shape[1]), probs, r.idx2label, 5, r.target_label) for f, r, (_, probs) in zip(frames, records, inputs)]
    return _plot_device([raw for raw, _ in inputs], tables_of, _resize_512)


def plot_top_preds_batch(records: list) -> list[np.ndarray]:
    """[record.plot()["top_preds"] for record in records] in one upload, one text launch and one copy back."""
    return frames_to_host(plot_top_preds_device(records)) if records else []
