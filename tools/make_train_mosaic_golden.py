#!/usr/bin/env python3
"""Generate tests/golden/train_mosaic.npz + train_mosaic_meta.json by RUNNING the reference's mosaic and the tail of its dataset
item on this repo's seeded raw samples (synth.synth_train_sample).

  PYTHONDONTWRITEBYTECODE=1 python3 tools/make_train_mosaic_golden.py [path to a checkout of the reference]

Needs a checkout of the reference (thawro/pytorch-human-pose); nothing of it is copied: the fixture holds arrays and numbers only.
The stub modules, the recorder and the binding of cv2.warpAffine are those of tools/make_train_input_golden.py, which is imported.

What is imported from the reference and therefore pinned by the fixture:
  * src.keypoints.datasets.coco.CocoKeypointsDataset.__getitem__ and .get_raw_mosaiced_data (an instance made without __init__, with
    get_raw_data / __len__ bound to the seeded samples): the mosaic draw and the draw of the three other tiles, the tile order and
    placement, the joints' scale / shift / truncation / zeroing, get_coco_joints, the mask threshold after the resize, and the order
    of all RNG draws of an item;
  * RandomAffineTransform / RandomHorizontalFlip, JointsGenerator, HeatmapGenerator as in the existing fixture.
What is NOT the reference's: `cv2.resize` and `cv2.warpAffine`.  cv2 is not installed where the fixtures are made, so the names are
bound to tests/cv_resize.resize (the restatement of OpenCV 4.x's 8-bit INTER_LINEAR resize stated in include/hhrnet.h) and to
oracle.transforms.warp_affine.  Parity of the resized and warped pixels with cv2 itself therefore stays UNPINNED.
"""
import hashlib
import json
import os
import random

import numpy as np

import make_train_input_golden as base  # noqa: E402  (sets up sys.path, the stubs and cv2.warpAffine, imports the reference)

import cv_resize  # noqa: E402
from train_mosaic_helpers import MosaicRecorder, canvas_sha, make_pool, pool_sha  # noqa: E402

coco = __import__("sys").modules["src.keypoints.datasets.coco"]
base.cv2.resize = cv_resize.resize

OUT_SIZE, RESOLUTIONS, NUM_KPTS, SIGMA, PROBABILITY = 64, [1 / 4, 1 / 2], 17, 2, 0.5
# [h, w, people, sample seed, mask holes]: smaller and larger than 64, a 2S x 2S one (the 2 x 2 mean), one without people
POOL = [[90, 70, 3, 11, 2], [128, 128, 2, 12, 1], [50, 200, 0, 13, -1], [64, 64, 1, 14, 0], [151, 97, 4, 15, 2]]
EMPTY = 2
# (tag, item index = tile 0, integer joints, wanted: the other tiles must hold the empty sample and a repeat, wanted flip, first RNG seed tried)
CASES = [("float_joints", 0, False, False, False, 201), ("integer_joints", 4, True, False, True, 301), ("empty_and_repeat", 1, False, True, False, 401)]


class _Dataset(coco.CocoKeypointsDataset):
    """get_raw_data / __len__ over the seeded pool; everything else is the reference's."""

    def get_raw_data(self, idx):
        image, mask, joints = self.pool[idx]
        annot = [dict(bbox=[0, 0, 1, 1], iscrowd=0, keypoints=person.reshape(-1).tolist(), num_keypoints=int((person[:, 2] > 0).sum()),
                      segmentation=None) for person in joints]
        return image, annot, mask

    def __len__(self):
        return len(self.pool)


def pick_seed(first, item, want_empty_and_repeat):
    """The first seed from `first` on whose item is a mosaic (random.random() < PROBABILITY) with the wanted other tiles."""
    for seed in range(first, first + 1000):
        random.seed(seed)
        if not random.random() < PROBABILITY:
            continue
        idxs = [item] + [random.randint(0, len(POOL) - 1) for _ in range(3)]
        if not want_empty_and_repeat or (EMPTY in idxs and len(set(idxs)) < 4):
            return seed, idxs
    raise SystemExit("no seed found")


def main():
    tf = base.KeypointsTransform(OUT_SIZE, RESOLUTIONS, **base.TRANSFORM)
    steps = tf.train.transforms[:2]  # RandomAffineTransform + RandomHorizontalFlip; not ToTensor / Normalize (the fixture records the uint8 image)
    hm_sizes = [int(r * OUT_SIZE) for r in RESOLUTIONS]
    seen = {}

    def transform(image, mask_list, joints_list):
        seen["canvas_sha256"], seen["canvas_shape"] = canvas_sha(image, mask_list[0]), list(image.shape)
        seen["joints_canvas"] = np.array(joints_list[0], np.float64)
        for t in steps:
            image, mask_list, joints_list = t(image, mask_list, joints_list)
        seen["joints_f"] = [np.array(j, np.float64) for j in joints_list]
        return np.ascontiguousarray(image), mask_list, joints_list

    out, meta_cases = {}, []
    for tag, item, integer, special, want_flip, first_seed in CASES:
        pool = make_pool(base.synth, POOL, NUM_KPTS, integer)
        before = pool_sha(pool)
        ds = object.__new__(_Dataset)  # no __init__: no files, no annotations
        ds.pool, ds.out_size, ds.mosaic_probability, ds.num_scales, ds.transform = pool, OUT_SIZE, PROBABILITY, len(hm_sizes), transform
        ds.hm_generators = [coco.HeatmapGenerator(NUM_KPTS, s, sigma=SIGMA) for s in hm_sizes]
        ds.joints_generators = [coco.JointsGenerator(s) for s in hm_sizes]
        seed, idxs = pick_seed(first_seed, item, special)
        while True:
            np.random.seed(seed)
            random.seed(seed)
            base.MATRICES.clear()
            with MosaicRecorder() as rec:
                image, heatmaps, mask_list, joints_list = ds[item]
            # a last-ulp difference in a restated dot product must not be able to flip int(): no coordinate near an integer
            jf = np.concatenate([j[..., :2].reshape(-1) for j in seen["joints_f"]])
            flipped = rec.draws[-1][0] == "random.random" and rec.draws[-1][1] < 0.5
            if (jf.size == 0 or np.abs(jf - np.round(jf)).min() > 1e-6) and flipped == want_flip:
                break
            seed, idxs = pick_seed(seed + 1, item, special)
        assert pool_sha(pool) == before, "the reference modified the pool"
        assert seen["canvas_shape"] == [2 * OUT_SIZE, 2 * OUT_SIZE, 3] and len(base.MATRICES) == len(hm_sizes) + 1
        assert [n for n, _ in rec.draws[:4]] == ["random.random"] + ["random.randint"] * 3
        assert [int(v) for _, v in rec.draws[1:4]] == idxs[1:]
        out[f"{tag}.image_u8"], out[f"{tag}.joints_canvas"] = image, seen["joints_canvas"]
        out[f"{tag}.mats"], out[f"{tag}.mat_image"] = np.stack(base.MATRICES[:-1]), base.MATRICES[-1]
        for i in range(len(hm_sizes)):
            assert set(np.unique(mask_list[i])) <= {0.0, 1.0} and heatmaps[i].dtype == np.float32
            out[f"{tag}.mask{i}"] = (mask_list[i] > 0).astype(np.uint8)
            out[f"{tag}.hm{i}"] = heatmaps[i]
            out[f"{tag}.joints_i{i}"] = joints_list[i]
        meta_cases.append(dict(tag=tag, item=item, integer_joints=integer, rng_seed=seed, tiles=idxs, draws=rec.draws, flip=bool(flipped),
                               pool_sha256=before, canvas_sha256=seen["canvas_sha256"], image_sha256=hashlib.sha256(image.tobytes()).hexdigest(),
                               people_on_canvas=int(len(seen["joints_canvas"])), people_per_stage=[int(len(j)) for j in joints_list]))
        print(tag, "seed", seed, "tiles", idxs, "flip", flipped, "draws", len(rec.draws), "people", len(seen["joints_canvas"]), [len(j) for j in joints_list])
    assert {c["flip"] for c in meta_cases} == {True, False}, "both flip outcomes are needed; pick other seeds"
    np.savez_compressed(os.path.join(base.OUT, "train_mosaic.npz"), **out)
    meta = dict(out_size=OUT_SIZE, hm_resolutions=RESOLUTIONS, num_kpts=NUM_KPTS, sigma=SIGMA, mosaic_probability=PROBABILITY, transform=base.TRANSFORM,
                pool=POOL, cases=meta_cases,
                resize="cv2.resize was bound to tests/cv_resize.resize (the project's restatement of OpenCV 4.x's 8-bit INTER_LINEAR resize, "
                       "include/hhrnet.h at hh_mosaic_u8_batch) and cv2.warpAffine to oracle.transforms.warp_affine: parity of the resized and "
                       "warped pixels with cv2 is UNPINNED; the mosaic draws, tile placement, joints, mask threshold, __getitem__'s order, the "
                       "transform, JointsGenerator and HeatmapGenerator are the reference's own code",
                raw_inputs="pool[i] = synth.synth_train_sample(h, w, people, sample_seed, num_kpts, holes), joints cast to int64 where "
                           "integer_joints; pool_sha256 over every image, mask and joints array in order; canvas_sha256 over the uint8 canvas "
                           "and the bool canvas mask as uint8")
    with open(os.path.join(base.OUT, "train_mosaic_meta.json"), "w") as f:
        json.dump(meta, f, indent=1)
    print("wrote", os.path.getsize(os.path.join(base.OUT, "train_mosaic.npz")), "bytes")


if __name__ == "__main__":
    main()
