"""Result container of one inference call.

Stands in for the non-plotting part of `/root/reference/src/keypoints/results.py:175-263`
(`InferenceKeypointsResult.from_preds`): stage-heatmap aggregation and decode run fused on
the GPU (hh_decode), the coordinate un-warp (results.py:158-171,189-201) on the host.
`plot_connections` / `plot` draw the pose overlay and the heatmap panels on the GPU (keypoints/visualization.py,
hh_render_poses_u8_batch, hh_heatmap_panels_u8); text is keypoints/text.py (hh_text_labels_u8_batch).  `calculate_OKS()` and the
per-image scores of `infer_images(score=...)` are keypoints/pose_score.py (hh_pose_score_batch).  The associative-embedding scatter
stays out of scope: it needs a rotated axis label and font sizes the text atlas does not have.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field

import numpy as np
import torch
from torch import Tensor

from .. import _lib
from .grouping import MPPEHeatmapParser


def transform_coords(kpts_coords: np.ndarray, center, scale, output_size) -> np.ndarray:
    """results.py:158-171 on an [..., 2] array (inverse of the resize affine, float64 like cv2)."""
    xy = np.ascontiguousarray(kpts_coords, dtype=np.float32).reshape(-1, 2)
    out = np.empty((xy.shape[0], 2), np.float64)
    _lib.check(_lib.load().hh_transform_coords(xy.ctypes.data, xy.shape[0], float(center[0]), float(center[1]), float(scale[0]),
                                               float(output_size[0]), float(output_size[1]), out.ctypes.data))
    return out.reshape(kpts_coords.shape).astype(kpts_coords.dtype)


def inverse_affine(center, scale, output_size) -> np.ndarray:
    """The 2x3 matrix `transform_coords` applies (hh_get_affine_transform with inverse = 1), row-major float64 [6]: what the DECODE form
    of hh_pose_score_batch takes per image."""
    M = np.empty(6, np.float64)
    _lib.check(_lib.load().hh_get_affine_transform(float(center[0]), float(center[1]), float(scale[0]), float(output_size[0]), float(output_size[1]), 1,
                                                   M.ctypes.data))
    return M


class KeypointsResult:
    """Validation-time result of one image (`results.py:70-155`): the stage heatmaps and tags of
    the net as they come out of `forward` (batch dim kept: [1,K,h,w]), decoded on demand by `set_preds()` with this result's
    own thresholds (validation uses max_num_people=20, det_thr=0.1, tag_thr=1.0, `keypoints/module.py:100-108`).  Coordinates
    are model-input pixels (no un-warp: the validation image IS the model input)."""

    def __init__(self, model_input_image: Tensor, kpts_heatmaps: list[Tensor], tags_heatmaps: Tensor, limbs, max_num_people: int = 30,
                 det_thr: float = 0.05, tag_thr: float = 0.5, parser: MPPEHeatmapParser | None = None):
        self.model_input_image = model_input_image
        self._kpts_heatmaps = kpts_heatmaps
        self._tags_heatmaps = tags_heatmaps
        self.num_kpts = kpts_heatmaps[0].shape[1]
        self.limbs = limbs
        self.max_num_people, self.det_thr, self.tag_thr = max_num_people, det_thr, tag_thr
        self.hm_parser = parser or MPPEHeatmapParser(self.num_kpts, max_num_people, det_thr, tag_thr)

    def _assign(self, joints: np.ndarray, scores: np.ndarray) -> None:
        self.kpts_coords, self.kpts_scores, self.kpts_tags, self.obj_scores = joints[..., :2], joints[..., 2], joints[..., 3:], scores

    def set_preds(self) -> None:
        """results.py:94-124: stage average, resize, parse -- fused in hh_decode."""
        out = self.hm_parser.decode_batch_device(self._kpts_heatmaps[0], self._kpts_heatmaps[1], [self._tags_heatmaps], adjust=True, refine=True)
        self._assign(*self.hm_parser.to_lists(*out)[0])

    @staticmethod
    def set_preds_batch(results: list["KeypointsResult"], stages: list[Tensor], tags: Tensor) -> None:
        """The same for every image of a batch in ONE hh_decode call (identical per-image results: images are independent)."""
        if not results:
            return
        parser = results[0].hm_parser
        for r, (j, s) in zip(results, parser.to_lists(*parser.decode_batch_device(stages[0], stages[1], [tags], adjust=True, refine=True))):
            r._assign(j, s)

    def plot(self) -> dict[str, np.ndarray]:
        from . import visualization as vis
        return {name: vis.to_host(figure) for name, figure in self._plot_device().items()}

    def _plot_device(self) -> dict[str, Tensor]:
        """results.py:126-155 after set_preds(): {"heatmaps": figure}, on the device.  Left, the connections overlay on the un-normalised model input
        (thr = det_thr, alpha = 0.8); right, per stage a one-row grid of that stage's maps clipped to 0..1 (stage 0 resized twice, as
        set_preds resizes it) followed, while the stage index is below the embedding dimension (1), by a one-row grid of the tags with
        min-max; the grids stacked, shrunk by 0.4 and put next to the overlay.  Everything per pixel runs on the GPU
        (hh_unnormalize_u8, hh_render_poses_u8_batch, hh_heatmap_panels_u8, hh_resize_u8_scaled, hh_resize_u8)."""
        from . import visualization as vis
        a, b = (t[0].float().contiguous() for t in self._kpts_heatmaps)
        tags = self._tags_heatmaps[0].float().contiguous()
        image = vis.unnormalize_device(self.model_input_image.to(a.device, torch.float32))
        table = vis.build_primitives(self.kpts_coords, self.kpts_scores, self.limbs, self.det_thr, "person", vis.DEFAULT_PALETTE, 0.8)
        connections = vis.render_frames_device([image], [table], 0.8)[0]
        grids = [([(vis.NESTED, m, None, vis.CLIP) for m in a], 1, 5), ([(vis.SINGLE, m, None, vis.MINMAX) for m in tags], 1, 5),
                 ([(vis.SINGLE, m, None, vis.CLIP) for m in b], 1, 5)]
        figure = vis.figure_device(image, grids, 0.4)
        return {"heatmaps": vis.stack_horizontally_device([connections, figure])}

    def plot_jpeg(self, quality: int = 90, subsampling="444") -> dict[str, bytes]:
        """plot() as the .jpg files the reference's callbacks save (src/base/callbacks.py:234,371): every figure encoded on the GPU from
        its device canvas (keypoints/jpeg.py), one encode call, only the compressed bytes copied back.  4:4:4 by default: the panels
        have thin coloured lines."""
        from .jpeg import encode_jpeg_device
        figures = self._plot_device()
        return dict(zip(figures, encode_jpeg_device(list(figures.values()), quality, subsampling)))


@dataclass
class InferenceKeypointsResult:
    raw_image: np.ndarray | None
    annot: list | None
    model_input_image: Tensor | None
    kpts_coords: np.ndarray  # [P,K,2] raw-image pixels
    kpts_scores: np.ndarray  # [P,K]
    kpts_tags: np.ndarray  # [P,K,E]
    obj_scores: np.ndarray  # [P]
    det_thr: float
    tag_thr: float
    limbs: list = field(default_factory=list)
    _stage_hms: list | None = None
    _tags: list | None = None
    rendered: np.ndarray | None = None  # infer_images(render=...): the finished overlay frame
    rendered_jpeg: bytes | None = None  # infer_images(render=dict(jpeg=...)): that frame as a JFIF stream, in place of `rendered`
    track_ids: np.ndarray | None = None  # with a PoseTracker: int32 [P], 0 = no track
    kpts_coords_smooth: np.ndarray | None = None  # with a PoseTracker: [P,K,2] raw-image pixels, One-Euro filtered
    oks: float | None = None  # infer_images(score="oks") or calculate_OKS(): image_OKS against `annot`, -1 without a labelled object
    object_oks: np.ndarray | None = None  # [T] unrounded OKS of every labelled object of `annot`, in annotation order
    kpt_oks: np.ndarray | None = None  # [T,K] exp(-e_k) per joint, -1 for an unlabelled joint
    target_matches: np.ndarray | None = None  # int32 [T]: the row of kpts_coords every labelled object took (the matching is the same
    # for both metrics: whichever of the OKS / PCKh scorings ran last wrote it, with equal contents)
    pckh: float | None = None  # infer_images(score="pckh"): image_PCKh against `annot` (objects carry "head_xyxy")
    object_pckh: np.ndarray | None = None  # [T], -1 for a head of size 0
    kpt_pckh: np.ndarray | None = None  # [T,K] 1 / 0 per joint, -1 for an unlabelled joint

    @property
    def raw_shape(self) -> tuple:
        """`raw_image.shape` without forming the pixels of a JPEG input."""
        return tuple(self.__dict__["_raw_image"].shape)

    @classmethod
    def from_preds(cls, raw_image, annot, model_input_image: Tensor, kpts_heatmaps: list[Tensor], tags_heatmaps: list[Tensor],
                   limbs, scale, center, det_thr: float = 0.05, tag_thr: float = 0.5, max_num_people: int = 30,
                   parser: MPPEHeatmapParser | None = None) -> "InferenceKeypointsResult":
        """results.py:203-263 for batch size 1 (the reference's inference wrapper is single-image)."""
        K = tags_heatmaps[0].shape[1]
        parser = parser or MPPEHeatmapParser(K, max_num_people, det_thr, tag_thr)
        img_h, img_w = model_input_image.shape[-2:]
        out = parser.decode_batch_device(kpts_heatmaps[0], kpts_heatmaps[1], tags_heatmaps, adjust=True, refine=True)
        joints, scores = parser.to_lists(*out)[0]
        coords = transform_coords(joints[..., :2], center, scale, (img_w, img_h))
        return cls(raw_image, annot, model_input_image, coords, joints[..., 2], joints[..., 3:], scores, det_thr, tag_thr, limbs,
                   kpts_heatmaps, tags_heatmaps)

    def _set_score(self, metric: str, value: float, obj: np.ndarray, kpt: np.ndarray, match: np.ndarray) -> None:
        if metric == "oks":
            self.oks, self.object_oks, self.kpt_oks, self.target_matches = value, obj, kpt, match
        else:
            self.pckh, self.object_pckh, self.kpt_pckh, self.target_matches = value, obj, kpt, match

    def calculate_OKS(self) -> float:
        """results.py:265-298: image_OKS of the predictions matched to the annotation's labelled objects; -1 for an annotation without
        one.  Computed on first call (hh_pose_score_host on this result's arrays, the F64 form) when the batch did not compute it
        (`infer_images(score="oks")`).  Unlike the reference nothing is reordered in place: the matched order is `target_matches`."""
        assert self.annot is not None, "Matching preds to targets is possible only when annotation is set"
        if self.oks is None:
            from . import pose_score as ps
            K = self.kpts_coords.shape[1]
            targets = ps.pack_targets([self.annot], "oks", num_kpts=K)
            if targets["t_off"][-1] == 0:
                self._set_score("oks", -1, np.zeros(0), np.zeros((0, K)), np.zeros(0, np.int32))
            else:
                out = ps.score_host(targets, preds=[(self.kpts_coords, self.obj_scores)], metric="oks", variances=ps.coco_variances(K))
                self._set_score("oks", float(out["value"][0]), out["obj"], out["kpt"], out["match"])
        return self.oks

    def plot_connections(self, color_mode: str = "person", alpha: float = 0.8) -> np.ndarray:
        """The reference's plot_connections on `raw_image` with thr = det_thr -> uint8 [h,w,3], drawn on the GPU."""
        from .visualization import plot_connections
        return plot_connections(self.raw_image, self.kpts_coords, self.kpts_scores, self.limbs, self.det_thr, color_mode, alpha)

    def _heatmaps_figure_device(self) -> Tensor:
        """results.py:317-328: the K stage-average maps and the K tag maps of the first embedding, both with min-max, each as a grid of
        two rows over the un-normalised model input, stacked and shrunk by 0.6 -> uint8 [h,w,3].  Painted on the GPU from the stage
        outputs (hh_heatmap_panels_u8); only the finished figure is copied to the host."""
        from . import visualization as vis
        a, b = (t[0].float().contiguous() for t in self._stage_hms)
        tags = self._tags[0][0].float().contiguous()
        image = vis.unnormalize_device(self.model_input_image.to(a.device, torch.float32))
        grids = [([(vis.AVERAGE, q, h, vis.MINMAX) for q, h in zip(a, b)], 2, 5), ([(vis.SINGLE, m, None, vis.MINMAX) for m in tags], 2, 5)]
        return vis.figure_device(image, grids, 0.6)

    def plot_heatmaps_figure(self) -> np.ndarray:
        from . import visualization as vis
        return vis.to_host(self._heatmaps_figure_device())

    def plot_jpeg(self, quality: int = 90, subsampling="444") -> dict[str, bytes]:
        """plot() as the .jpg files the reference's perform_inference saves (src/base/datasets/base.py:140): the same figures, drawn and
        encoded on the GPU (keypoints/jpeg.py) in one encode call; only the compressed bytes are copied back.  4:4:4 by default: the
        overlays and panels have thin coloured lines."""
        from . import visualization as vis
        from .jpeg import encode_jpeg_device
        image = np.ascontiguousarray(self.raw_image, dtype=np.uint8)
        table = vis.build_primitives(self.kpts_coords, self.kpts_scores, self.limbs, self.det_thr, "person", vis.DEFAULT_PALETTE, 0.8)
        figures = {"connections": vis.render_frames_device([image], [table], 0.8)[0]}
        if self._stage_hms is not None and self._tags is not None and self.model_input_image is not None:
            figures["heatmaps"] = self._heatmaps_figure_device()
        return dict(zip(figures, encode_jpeg_device(list(figures.values()), quality, subsampling)))

    def plot(self) -> dict[str, np.ndarray]:
        """results.py:300-339 as far as it is built here: {"connections": ...} and, when the result holds its stage maps, tags and
        model input, {"heatmaps": ...} (plot_heatmaps_figure).  The reference's "associative_embedding" entry is a matplotlib scatter:
        out of scope (a rotated axis label and font sizes the text atlas does not have).  The reference also prints calculate_OKS()
        here when an annotation is set; call it yourself (`result.calculate_OKS()`, or `infer_images(score="oks")`)."""
        plots = {"connections": self.plot_connections()}
        if self._stage_hms is not None and self._tags is not None and self.model_input_image is not None:
            plots["heatmaps"] = self.plot_heatmaps_figure()
        return plots

    # visualisation-only views of the reference (resized maps on the host); not on the hot path
    @property
    def kpts_heatmaps(self) -> np.ndarray:
        f = torch.nn.functional.interpolate
        h, w = self.model_input_image.shape[-2:]
        a, b = self._stage_hms
        avg = (f(a, size=list(b.shape[-2:]), mode="bilinear", align_corners=False) + b) / 2
        return f(avg, size=[h, w], mode="bilinear", align_corners=False)[0].cpu().numpy()

    @property
    def tags_heatmaps(self) -> np.ndarray:
        f = torch.nn.functional.interpolate
        h, w = self.model_input_image.shape[-2:]
        return f(self._tags[0], size=[h, w], mode="bilinear", align_corners=False)[0].cpu().numpy()


def _raw_image(self):
    """The input image.  Of a JPEG input (a jpeg.JpegImage: only its bytes went to the device) the pixels are formed here on first
    access by the host rule, which is bit-identical to the device's, and kept."""
    raw = self.__dict__.get("_raw_image")
    if hasattr(raw, "stage"):  # a jpeg.JpegImage
        from .jpeg import decode_jpeg_host
        raw = self.__dict__["_raw_image"] = decode_jpeg_host(raw.data)
    return raw


# (installed behind the dataclass decorator: the generated __init__ assigns through the setter)
InferenceKeypointsResult.raw_image = property(_raw_image, lambda self, value: self.__dict__.__setitem__("_raw_image", value))
