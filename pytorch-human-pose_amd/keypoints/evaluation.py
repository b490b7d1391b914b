"""COCO result packing of the evaluation harness (`src/keypoints/bin/eval.py:18-49`).

The packing and the image-sharded loop live here.  AP itself is computed by pycocotools 2.0.7 in the reference (`bin/eval.py:52-65`),
a third-party evaluator that is not in this image; `keypoints.coco_eval` restates it, on the host and on the device, and
`evaluate_images(..., gt_annotations=..., score_device=...)` runs the device form on the gathered list.
"""
from __future__ import annotations

from pathlib import Path

import numpy as np

from .distributed import gather_results, shard_range


def image_id_from_path(image_filepath: str) -> int:
    """bin/eval.py:23: COCO file stems are zero-padded image ids."""
    return int(Path(image_filepath).stem.lstrip("0"))


def pack_coco_results(image_id: int, kpts_coords: np.ndarray, obj_scores: np.ndarray) -> list[dict]:
    """bin/eval.py:27-48: one entry per person, keypoints = [x, y, 1] * K (float64), score = the person's score
    (`scores.mean()` of a scalar in the reference, i.e. the score itself, as a python float)."""
    results = []
    for i in range(len(obj_scores)):
        kpts = kpts_coords[i]
        coco_kpts = np.zeros((len(kpts) * 3,))
        coco_kpts[::3] = kpts[:, 0]
        coco_kpts[1::3] = kpts[:, 1]
        coco_kpts[2::3] = 1
        results.append({"image_id": int(image_id), "category_id": 1, "keypoints": coco_kpts.tolist(),
                        "score": np.asarray(obj_scores[i]).mean().item()})
    return results


def evaluate_images(model, images, image_ids, rank: int = 0, world_size: int = 1, multi_scale=None, batch: int = 32, gt_annotations=None,
                    score_device=None, image_scores: bool = False):
    """evaluate_dataset (bin/eval.py:18-49) over in-memory images, sharded by image across ranks (§8e: contiguous
    slices, no data-path collective; the packed lists are gathered to rank 0, other ranks get None).
    `multi_scale` = tuple of scales -> `model.call_multi_scale` (the cfg-4 extension) instead of `model(...)`.
    `batch` > 1 routes both cases through `model.infer_images` (identical per-image results, one forward and one decode per
    shape bucket; with `multi_scale`, `infer_images(scales=multi_scale)`: the forwards of plan_multi_scale and one fused
    aggregation per stage); `batch` = 1 is the reference's image-by-image loop.
    With both `gt_annotations` (the "annotations" list of a person_keypoints json) and `score_device` (e.g. "cuda:0") rank 0 returns
    (packed list, stats): the list scored over `image_ids` by `coco_eval.evaluate_device`, the `eval_coco` step on the device; the
    other ranks return (None, None).  Without them the return value is the packed list alone, as before.
    `image_scores=True` (needs `gt_annotations`): every image is also scored against its own annotations as the reference's
    calculate_OKS scores it (keypoints/pose_score.py; with `batch` > 1 on the device, one hh_pose_score_batch per batch behind its
    decode), and the return value gains two more elements: {image_id: oks} (-1 for an image without a labelled object) and the float64
    [K] mean of the per-joint term exp(-e_k) over all scored targets that label the joint (NaN for a joint none labels): the "which
    joint is weak" table.  Other ranks get None for both."""
    if image_scores and gt_annotations is None:
        raise ValueError("evaluate_images: image_scores=True needs gt_annotations")
    local, scored = [], []
    mine = list(shard_range(len(images), rank, world_size))
    annots = [None] * len(images)
    if image_scores:
        by_image: dict = {}
        for a in gt_annotations:
            by_image.setdefault(int(a["image_id"]), []).append(a)
        annots = [by_image.get(int(i), []) for i in image_ids]

    def collect(idx, res):
        local.extend(pack_coco_results(image_ids[idx], res.kpts_coords, res.obj_scores))
        if image_scores:
            oks = res.calculate_OKS()  # (the stored value where the batch computed it)
            lab = res.kpt_oks >= 0
            scored.append({"image_id": int(image_ids[idx]), "oks": float(oks), "kpt_sum": np.where(lab, res.kpt_oks, 0.0).sum(0).tolist(),
                           "kpt_cnt": lab.sum(0).tolist()})

    if batch <= 1:
        for idx in mine:
            collect(idx, model.call_multi_scale(images[idx], annots[idx], multi_scale) if multi_scale else model(images[idx], annots[idx]))
    else:  # batched behind the same per-image results: shape buckets of up to `batch` images per forward + decode
        kw = {"scales": multi_scale} if multi_scale else {}
        if image_scores:
            kw.update(annots=[annots[i] for i in mine], score="oks")
        for idx, res in zip(mine, model.infer_images([images[i] for i in mine], max_batch=batch, **kw)):
            collect(idx, res)
    packed = gather_results(local)
    extra = ()
    if image_scores:
        rows = gather_results(scored)
        extra = (None, None)
        if rows is not None:
            cnt = np.sum([r["kpt_cnt"] for r in rows], axis=0) if rows else np.zeros(0)
            tot = np.sum([r["kpt_sum"] for r in rows], axis=0) if rows else np.zeros(0)
            with np.errstate(invalid="ignore", divide="ignore"):
                extra = ({r["image_id"]: r["oks"] for r in rows}, np.asarray(tot, np.float64) / np.asarray(cnt, np.float64))
    if gt_annotations is None or score_device is None:
        return (packed,) + extra if image_scores else packed
    if packed is None:
        return (None, None) + extra
    from .coco_eval import evaluate_device
    return (packed, evaluate_device(gt_annotations, packed, score_device, img_ids=[int(i) for i in image_ids])[2]) + extra
