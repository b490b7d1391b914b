"""Per-image OKS and PCKh against annotations: the reference's `match_preds_to_targets` (keypoints/results.py:21-43), `object_OKS` /
`image_OKS` (keypoints/datasets/coco.py:489-535) and `object_PCKh` / `image_PCKh` (keypoints/datasets/mpii.py), scored on the device
behind hh_decode (hh_pose_score_batch; the rule is written at that entry point in include/hhrnet.h).  `pack_targets` builds the target
tables from annotations on the host, `score_device` is the one launch per batch, `score_host` runs the same text compiled for the host
(the functions with the reference's names go through it; tests, tools).  Opt-in everywhere: without `score=` every path runs as before.

Two stated differences from the reference: sums run in ascending order (numpy sums pairwise from 8 elements up), and the matched order
is returned instead of reordering the predictions in place.  Parity of `polygon_area` with cv2.contourArea is UNPINNED (cv2 is absent
where the fixtures are made)."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from .. import _lib

MAX_T, MAX_P, MAX_K = (_lib.const("POSE_" + k) for k in ("MAX_T", "MAX_P", "MAX_K"))
PRED_DECODE, PRED_F64 = _lib.const("POSE_PRED_DECODE"), _lib.const("POSE_PRED_F64")
METRICS = {"oks": _lib.const("POSE_METRIC_OKS"), "pckh": _lib.const("POSE_METRIC_PCKH")}
NONFINITE, NO_PRED = _lib.const("POSE_NONFINITE"), _lib.const("POSE_NO_PRED")
SPACING = float(np.spacing(1))  # 2^-52: what object_OKS adds to the polygon area
# coco.py:484-486: (2 k_i)^2 of the COCO keypoint constants, formed as the reference forms them
OKS_VARIANCES = (np.array([26, 25, 25, 35, 35, 79, 79, 72, 72, 62, 62, 107, 107, 87, 87, 89, 89]) / 1000 * 2) ** 2


def _c(a, dtype):
    return np.ascontiguousarray(a, dtype=dtype)


def polygon_area(polygon) -> float:
    """hh_polygon_area of one flat [x0, y0, x1, y1, ...] polygon: the exact int64 shoelace of the coordinates truncated toward zero."""
    xy = _c(polygon, np.float64).reshape(-1)
    if xy.size % 2:
        raise ValueError("a polygon needs an even number of coordinates")
    out = np.zeros(1, np.float64)
    _lib.check(_lib.load().hh_polygon_area(xy.ctypes.data if xy.size else None, xy.size // 2, out.ctypes.data))
    return float(out[0])


def object_area(segmentation) -> float:
    """sum(contourArea(polygon)) + np.spacing(1) of one object's `segmentation`; a missing or empty one gives 2^-52."""
    if isinstance(segmentation, dict):
        raise ValueError("pose_score: a run-length (iscrowd) segmentation on a labelled object cannot be scored (the reference cannot either)")
    area = 0.0
    for poly in segmentation or []:
        area = area + polygon_area(poly)
    return area + SPACING


def head_size(head_xyxy) -> float:
    """mpii.py:15-16."""
    xmin, ymin, xmax, ymax = head_xyxy
    return float(((xmax - xmin) ** 2 + (ymax - ymin) ** 2) ** 0.5)


def labelled_objects(annot) -> list[int]:
    """calculate_OKS's filter: the indices of the annotation's objects with any v > 0, in annotation order."""
    return [j for j, obj in enumerate(annot) if np.any(np.array(obj["keypoints"]).reshape([-1, 3])[:, 2] > 0)]


def pack_targets(annots, metric: str = "oks", head_boxes=None, num_kpts: int | None = None) -> dict:
    """The target tables of a batch: `annots[i]` is image i's annotation (a list of COCO-style objects with "keypoints" and
    "segmentation") or None (no targets: the image is not scored).  Targets are the objects with any v > 0, in annotation order.
    metric "pckh": the head box (xmin, ymin, xmax, ymax) of object j of image i is `head_boxes[i][j]`, or the object's "head_xyxy".
    -> dict(t_off int32 [B+1], t_xyv [T,K,3], t_area [T], t_head [T] as float64, K).  Refuses by name: a run-length segmentation on a
    labelled object, more than HH_POSE_MAX_T targets in an image, K over HH_POSE_MAX_K, objects of different K, non-finite values."""
    if metric not in METRICS:
        raise ValueError(f"metric must be one of {sorted(METRICS)}, got {metric!r}")
    rows, areas, heads, off = [], [], [], [0]
    K = num_kpts
    for i, annot in enumerate(annots):
        for j in labelled_objects(annot) if annot is not None else []:
            obj = annot[j]
            kp = _c(obj["keypoints"], np.float64).reshape(-1, 3)
            if K is None:
                K = len(kp)
            if len(kp) != K:
                raise ValueError(f"pose_score: image {i}: object {j} has {len(kp)} keypoints, expected {K}")
            if not np.isfinite(kp).all():
                raise ValueError(f"pose_score: image {i}: object {j} has a non-finite keypoint value")
            rows.append(kp)
            if metric == "oks":
                try:
                    areas.append(object_area(obj.get("segmentation")))
                except ValueError as e:
                    raise ValueError(f"image {i}: object {j}: {e}") from None
                heads.append(0.0)
            else:
                box = head_boxes[i][j] if head_boxes is not None else obj["head_xyxy"]
                areas.append(SPACING)
                heads.append(head_size(box))
        if len(rows) - off[-1] > MAX_T:
            raise ValueError(f"pose_score: image {i} has {len(rows) - off[-1]} labelled objects, over HH_POSE_MAX_T ({MAX_T}): refused, not capped")
        off.append(len(rows))
    if K is None:
        raise ValueError("pose_score: no labelled object to take the number of keypoints from: pass num_kpts")
    if not 1 <= K <= MAX_K:
        raise ValueError(f"pose_score: {K} keypoints, outside 1..HH_POSE_MAX_K ({MAX_K})")
    return {"t_off": np.asarray(off, np.int32), "t_xyv": _c(rows, np.float64).reshape(-1, K, 3), "t_area": _c(areas, np.float64).reshape(-1),
            "t_head": _c(heads, np.float64).reshape(-1), "K": int(K)}


def make_targets(t_xyv, t_off=None, t_area=None, t_head=None) -> dict:
    """Target tables from arrays (tests, tools): one image unless `t_off` is given; area defaults to 1, head to 0."""
    t_xyv = _c(t_xyv, np.float64)
    T, K = t_xyv.shape[:2]
    return {"t_off": np.asarray([0, T] if t_off is None else t_off, np.int32), "t_xyv": t_xyv,
            "t_area": np.ones(T) if t_area is None else _c(t_area, np.float64).reshape(T),
            "t_head": np.zeros(T) if t_head is None else _c(t_head, np.float64).reshape(T), "K": int(K)}


def pack_preds(preds, K: int) -> dict:
    """The F64 prediction tables of a batch: `preds[i]` = (xy [P,K,2], scores [P]) of image i, widened to float64 as they are."""
    off = np.cumsum([0] + [len(s) for _, s in preds]).astype(np.int32)
    xy = [_c(x, np.float64).reshape(-1, K, 2) for x, _ in preds]
    sc = [_c(s, np.float64).reshape(-1) for _, s in preds]
    return {"p_off": off, "p_xy": np.concatenate(xy) if xy else np.zeros((0, K, 2)), "p_score": np.concatenate(sc) if sc else np.zeros(0)}


def _outputs_host(B: int, T: int, K: int) -> dict:
    return {"value": np.empty(B, np.float64), "obj": np.empty(T, np.float64), "kpt": np.empty((T, K), np.float64), "match": np.empty(T, np.int32),
            "status": np.empty(B, np.int32)}


_EMPTY = np.zeros(8, np.float64)  # what an empty table points at (non-null, aligned, never read)


def _ptr(a):
    return None if a is None else a.ctypes.data if a.size else _EMPTY.ctypes.data


def score_host(targets: dict, preds=None, decode=None, inv_affine=None, metric: str = "oks", variances=OKS_VARIANCES, alpha: float = 0.5) -> dict:
    """hh_pose_score_host: the device's text compiled for the host.  `preds` = [(xy [P,K,2], scores [P]), ...] per image (the F64 form)
    or `decode` = (joints [B,M,K,3+E] float32, scores [B,M] float32, num [B], flags [B] or None) numpy arrays with `inv_affine` [B,6]
    (the DECODE form).  -> dict(value [B], obj [T], kpt [T,K], match [T], status [B])."""
    K, B = targets["K"], len(targets["t_off"]) - 1
    T = int(targets["t_off"][-1]) if B >= 0 and len(targets["t_off"]) else 0
    out = _outputs_host(max(B, 0), max(T, 0), K)
    var = _c(variances, np.float64).reshape(-1)
    if len(var) < K:
        raise ValueError(f"{len(var)} variances for {K} keypoints")
    keep = [var, targets]
    if decode is not None:
        joints, scores, num = _c(decode[0], np.float32), _c(decode[1], np.float32), _c(decode[2], np.int32)
        flags = None if len(decode) < 4 or decode[3] is None else _c(decode[3], np.int32)
        M = _c(inv_affine, np.float64).reshape(-1, 6)
        W = joints.shape[3]
        args = (PRED_DECODE, METRICS[metric], B, K, _ptr(joints), joints.shape[1] * K * W, K * W, W, _ptr(scores), scores.shape[1], _ptr(num),
                None if flags is None else _ptr(flags), joints.shape[1], _ptr(M), None, None, None)
        keep += [joints, scores, num, flags, M]
    else:
        p = pack_preds(preds, K)
        args = (PRED_F64, METRICS[metric], B, K, None, 0, 0, 0, None, 0, None, None, 0, None, _ptr(p["p_off"]), _ptr(p["p_xy"]), _ptr(p["p_score"]))
        keep.append(p)
    _lib.check(_lib.load().hh_pose_score_host(*args, _ptr(targets["t_off"]), _ptr(targets["t_xyv"]), _ptr(targets["t_area"]), _ptr(targets["t_head"]),
                                              _ptr(var), float(alpha), *(_ptr(out[k]) for k in ("value", "obj", "kpt", "match", "status"))))
    return out


@dataclass
class DeviceScore:
    """The outputs of one hh_pose_score_batch on the device: `blob` (uint8) holds value | obj | kpt | match | status back to back, so
    that they cross to the host as ONE array; `split` cuts a host copy of it into the named arrays."""
    blob: torch.Tensor
    B: int
    T: int
    K: int
    keep: tuple = ()  # what the launch reads, alive until it has run
    t_off: np.ndarray | None = None  # the targets' offsets: image i's rows of obj / kpt / match are t_off[i] .. t_off[i+1]-1

    @staticmethod
    def layout(B: int, T: int, K: int):
        sizes = (("value", np.float64, (B,)), ("obj", np.float64, (T,)), ("kpt", np.float64, (T, K)), ("match", np.int32, (T,)), ("status", np.int32, (B,)))
        at, out = 0, {}
        for name, dt, shape in sizes:  # (the fp64 arrays first: every offset stays a multiple of its element size)
            out[name] = (at, dt, shape)
            at += int(np.prod(shape)) * np.dtype(dt).itemsize
        return out, max(at, 8)

    @staticmethod
    def capacity(nbytes: int) -> int:
        """The size the blob is allocated with: the next power of two from 4 KB up, so that the shapes a pipeline sees (and keeps pinned
        result buffers for) are a handful of classes, not one per target count.  The layout inside does not depend on it."""
        cap = 4096
        while cap < nbytes:
            cap *= 2
        return cap

    def split(self, host_blob) -> dict:
        raw = host_blob.numpy() if isinstance(host_blob, torch.Tensor) else np.asarray(host_blob)
        lay, _ = self.layout(self.B, self.T, self.K)
        return {k: raw[at:at + int(np.prod(shape)) * np.dtype(dt).itemsize].view(dt).reshape(shape).copy() for k, (at, dt, shape) in lay.items()}

    def to_host(self) -> dict:
        return self.split(self.blob.cpu())


class TableStage:
    """A pinned host buffer for the tables of score_device calls that follow each other, grown when a call needs more and otherwise
    reused: allocating page-locked memory per call costs more than the launch.  The caller guarantees that the copy of the previous
    call that used it has finished (a pipeline slot whose previous batch has been collected)."""

    def __init__(self):
        self.buffer = None

    def take(self, nbytes: int) -> torch.Tensor:
        if self.buffer is None or self.buffer.numel() < nbytes:
            self.buffer = torch.empty(DeviceScore.capacity(nbytes), dtype=torch.uint8).pin_memory()
        return self.buffer


def _upload(arrays: list, device, stage: TableStage | None = None) -> tuple:
    """The host arrays back to back (each at a multiple of 8 bytes) in ONE pinned buffer (`stage`'s, or a new one) and ONE host ->
    device copy on the current stream -> (device addresses, device tensor, pinned tensor)."""
    offs, at = [], 0
    for a in arrays:
        offs.append(at)
        at += (a.nbytes + 7) // 8 * 8
    total = max(at, 8)
    host = stage.take(total) if stage is not None else torch.empty(total, dtype=torch.uint8).pin_memory()
    view = host.numpy()
    for a, o in zip(arrays, offs):
        view[o:o + a.nbytes] = a.reshape(-1).view(np.uint8)
    dev = host[:total].to(device, non_blocking=True)
    return [dev.data_ptr() + o for o in offs], dev, host


def score_device(targets: dict, decode=None, inv_affine=None, preds=None, metric: str = "oks", variances=OKS_VARIANCES, alpha: float = 0.5,
                 device=None, stage: TableStage | None = None) -> DeviceScore:
    """ONE hh_pose_score_batch on the current stream, no host synchronisation.  `decode` = the device tensors of
    MPPEHeatmapParser.decode_batch_device (joints, scores, num, flags), read in place, with `inv_affine` [B,6] float64 on the host (the
    DECODE form; `keypoints.results.inverse_affine`), or `preds` = [(xy, scores), ...] on the host (the F64 form, uploaded with the
    targets).  The target tables travel in one pinned host -> device copy in front of the launch (from `stage`'s buffer if one is
    given, see TableStage).  The output blob's size is rounded up (DeviceScore.capacity).  There is no CPU fallback."""
    K, B = targets["K"], len(targets["t_off"]) - 1
    T = int(targets["t_off"][-1])
    var = _c(variances, np.float64).reshape(-1)
    if len(var) < K:
        raise ValueError(f"{len(var)} variances for {K} keypoints")
    lib = _lib.load()
    tabs = [targets["t_off"], targets["t_xyv"], targets["t_area"], targets["t_head"]]
    if decode is not None:
        joints, scores, num, flags = decode
        device = joints.device
        if not joints.is_cuda or joints.dtype != torch.float32 or scores.dtype != torch.float32 or num.dtype != torch.int32:
            raise _lib.HHError("pose_score.score_device needs the decode's device tensors: there is no CPU path")
        if joints.shape[0] != B or joints.shape[2] != K:
            raise ValueError(f"joints {tuple(joints.shape)} against {B} images of {K} keypoints")
        M = _c(inv_affine, np.float64).reshape(B, 6)
        tabs.append(M)
    else:
        device = torch.device(device)
        if device.type != "cuda":
            raise _lib.HHError("pose_score.score_device needs a CUDA/HIP device: there is no CPU path")
        p = pack_preds(preds, K)
        tabs += [p["p_off"], p["p_xy"], p["p_score"]]
    with torch.cuda.device(device):
        addr, dev_tabs, pinned = _upload(tabs, device, stage)
        lay, nbytes = DeviceScore.layout(B, T, K)
        blob = torch.empty(DeviceScore.capacity(nbytes), dtype=torch.uint8, device=device)
    outs = [blob.data_ptr() + lay[k][0] for k in ("value", "obj", "kpt", "match", "status")]
    host_t = [_ptr(a) for a in tabs[:4]]
    if decode is not None:
        args = (PRED_DECODE, METRICS[metric], B, K, joints.data_ptr(), joints.stride(0), joints.stride(1), joints.stride(2), scores.data_ptr(),
                scores.stride(0), num.data_ptr(), _lib.ptr(flags), joints.shape[1], addr[4], _ptr(tabs[4]), None, None, None, None)
    else:
        args = (PRED_F64, METRICS[metric], B, K, None, 0, 0, 0, None, 0, None, None, 0, None, None, addr[4], _ptr(tabs[4]), addr[5], addr[6])
    _lib.launch(device, lib.hh_pose_score_batch, *args, addr[0], host_t[0], addr[1], host_t[1], addr[2], host_t[2], addr[3], host_t[3], _ptr(var),
                float(alpha), *outs)
    return DeviceScore(blob, B, T, K, keep=(dev_tabs, pinned, decode), t_off=targets["t_off"])


def config() -> dict:
    out = np.zeros(4, np.int32)
    _lib.check(_lib.load().hh_pose_score_config(out.ctypes.data))
    return dict(zip(("threads", "lds_bytes_max", "max_targets", "max_preds"), (int(v) for v in out)))


# ---------------------------------------------------------------------------------------------- the reference's functions
def coco_variances(K: int) -> np.ndarray:
    """OKS_VARIANCES for the 17 COCO keypoints; any other K is refused (the constants belong to those joints: pass `variances` to
    score_host / score_device for another skeleton), as the reference's object_OKS fails to broadcast there."""
    if K != len(OKS_VARIANCES):
        raise ValueError(f"pose_score: the OKS constants are those of the {len(OKS_VARIANCES)} COCO keypoints, not of {K}: pass your own variances to "
                         "score_host / score_device")
    return OKS_VARIANCES


def _one_image(pred_xy, pred_scores, target_kpts, target_vis, metric="oks", area=None, head=None, alpha=0.5, variances=OKS_VARIANCES) -> dict:
    target_kpts, target_vis = np.asarray(target_kpts), np.asarray(target_vis)
    T, K = target_kpts.shape[:2]
    xyv = np.concatenate([_c(target_kpts[..., :2], np.float64), _c(target_vis, np.float64)[..., None]], axis=-1)
    var = np.ones(K) if variances is None or len(variances) < K else variances
    return score_host(make_targets(xyv, None, area, head), preds=[(np.asarray(pred_xy)[..., :2], pred_scores)], metric=metric, variances=var, alpha=alpha)


def match_preds_to_targets(pred_joints: np.ndarray, pred_scores: np.ndarray, target_kpts: np.ndarray, target_visibilities: np.ndarray) -> list[int]:
    """results.py:21-43: for every target the index of the prediction it takes."""
    if len(target_kpts) == 0:
        return []
    if len(pred_scores) == 0:
        return [-1] * len(target_kpts)
    out = _one_image(pred_joints, pred_scores, target_kpts, target_visibilities, variances=None)
    if out["status"][0]:
        raise _lib.HHError("match_preds_to_targets: a predicted coordinate or score is not finite")
    return [int(m) for m in out["match"]]


def _pairs(pred_kpts, target_kpts, target_vis, metric, areas=None, heads=None, alpha=0.5) -> np.ndarray:
    """obj of prediction j against target j for every j with a labelled joint (one image of one pair each), -1 for the others."""
    pred_kpts, target_kpts, target_vis = np.asarray(pred_kpts), np.asarray(target_kpts), np.asarray(target_vis)
    n = len(target_kpts)
    res = np.full(n, -1.0)
    use = [j for j in range(n) if target_vis[j].sum() > 0]
    if not use:
        return res
    K = target_kpts.shape[1]
    xyv = np.concatenate([_c(target_kpts[use][..., :2], np.float64), _c(target_vis[use], np.float64)[..., None]], axis=-1)
    tg = make_targets(xyv, np.arange(len(use) + 1), None if areas is None else [areas[j] for j in use], None if heads is None else [heads[j] for j in use])
    out = score_host(tg, preds=[(pred_kpts[j][None, :, :2], np.zeros(1)) for j in use], metric=metric, alpha=alpha,
                     variances=coco_variances(K) if metric == "oks" else np.ones(K))  # (PCKh reads no variance)
    if out["status"].any():
        raise _lib.HHError("pose_score: a predicted coordinate is not finite")
    res[use] = out["obj"]
    return res


def object_OKS(pred_kpts: np.ndarray, target_kpts: np.ndarray, target_vis: np.ndarray, obj_polygons) -> float:
    """coco.py:489-514 for one (prediction, target) pair; -1 for a target without a labelled joint."""
    if np.asarray(target_vis).sum() <= 0:
        return -1
    return float(_pairs(pred_kpts[None], np.asarray(target_kpts)[None], np.asarray(target_vis)[None], "oks", [object_area(obj_polygons)])[0])


def image_OKS(pred_kpts: np.ndarray, target_kpts: np.ndarray, target_vis: np.ndarray, seg_polygons) -> float:
    """coco.py:517-535: prediction j against target j, round(3), the mean of the values that are not -1 (ascending), else -1."""
    oks = _pairs(pred_kpts, target_kpts, target_vis, "oks", [object_area(s) for s in seg_polygons])
    vals = [float(np.rint(v * 1000.0) / 1000.0) for v in oks if v != -1]
    return sum(vals, 0.0) / len(vals) if vals else -1


def object_PCKh(pred_kpts: np.ndarray, target_kpts: np.ndarray, target_vis: np.ndarray, head_xyxy, alpha: float = 0.5) -> float:
    """mpii.py:6-28, in float64."""
    if np.asarray(target_vis).sum() <= 0 or head_size(head_xyxy) == 0:
        return -1
    return float(_pairs(pred_kpts[None], np.asarray(target_kpts)[None], np.asarray(target_vis)[None], "pckh", None, [head_size(head_xyxy)], alpha)[0])


def image_PCKh(alpha: float, pred_kpts: np.ndarray, target_kpts: np.ndarray, target_vis: np.ndarray, head_coords) -> float:
    """mpii.py:31-53."""
    n = len(head_coords)
    vals = [float(v) for v in _pairs(pred_kpts[:n], target_kpts[:n], target_vis[:n], "pckh", None, [head_size(h) for h in head_coords], alpha) if v != -1]
    return sum(vals, 0.0) / len(vals) if vals else -1
