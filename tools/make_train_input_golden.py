#!/usr/bin/env python3
"""Generate tests/golden/train_input.npz + train_input_meta.json by RUNNING the reference's train-time transform and target
generators on this repo's seeded raw samples (synth.synth_train_sample).

  PYTHONDONTWRITEBYTECODE=1 python3 tools/make_train_input_golden.py [path to a checkout of the reference]

Needs a checkout of the reference (thawro/pytorch-human-pose); nothing of it is copied: the fixture holds arrays and numbers only.

What is imported from the reference and therefore pinned by the fixture:
  * src.keypoints.transforms.KeypointsTransform -> RandomAffineTransform.__call__ / _get_affine_matrix / _affine_joints and
    RandomHorizontalFlip.__call__: the RNG draws and their order, the matrices, the transformed and flipped joints, the mask
    threshold, the flip of image and masks;
  * src.keypoints.datasets.coco.JointsGenerator, HeatmapGenerator, collate_fn.
What is NOT the reference's: `cv2.warpAffine`.  cv2 is not installed where the fixtures are made, so the name is bound to
oracle.transforms.warp_affine, the project's restatement of OpenCV 4.9's 8-bit INTER_LINEAR path.  Parity of the warped pixels
with cv2 itself therefore stays UNPINNED here exactly as for hh_preprocess_u8; everything around the warp is the reference's code.

The modules the reference imports at module level and that are absent (cv2, torchvision, albumentations, pycocotools, torchinfo,
colorlog, ...) and the reference's own logger / plotting packages are replaced by permissive stubs: none of their attributes is
used by the code that runs here (ToTensor / Normalize of the transform are not run: the fixture records the uint8 image).
"""
import hashlib
import importlib
import importlib.abc
import importlib.machinery
import json
import os
import random
import sys
import types

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
sys.dont_write_bytecode = True
sys.path.insert(0, REF)
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))  # train_input_helpers.Recorder: the same recorder the tests use
OUT = os.path.join(REPO, "tests", "golden")


# ------------------------------------------------------------------ stubs for what cannot be imported here
class _StubMeta(type):
    def __getattr__(cls, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return _Stub

    def __or__(cls, other):
        return cls

    __ror__ = __or__

    def __getitem__(cls, item):
        return cls


class _Stub(metaclass=_StubMeta):
    def __init__(self, *a, **k):
        pass

    def __call__(self, *a, **k):
        return self

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return _Stub()


class _StubModule(types.ModuleType):
    __path__: list = []

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return _Stub


REF_OWN_STUBS = ("src.logger", "src.keypoints.visualization", "src.base.visualization", "src.utils.image")


class _StubFinder(importlib.abc.MetaPathFinder, importlib.abc.Loader):
    """Last on sys.meta_path: reached only for what no real finder has.  Third-party names become stubs; of the reference's own
    modules only the logger / plotting ones listed above do (they are placed FIRST for those, see below)."""

    def __init__(self, own_only):
        self.own_only = own_only

    def find_spec(self, name, path=None, target=None):
        own = any(name == p or name.startswith(p + ".") for p in REF_OWN_STUBS)
        if self.own_only != own or (not own and (name == "src" or name.startswith("src.") or name.startswith("_"))):
            return None
        return importlib.machinery.ModuleSpec(name, self, is_package=True)

    def create_module(self, spec):
        return _StubModule(spec.name)

    def exec_module(self, module):
        pass


import torch  # noqa: E402,F401  (the real one, with everything it imports lazily, before the permissive finder exists)

from oracle import transforms as otf  # noqa: E402

synth = importlib.import_module("pytorch-human-pose_amd.synth")
from train_input_helpers import Recorder  # noqa: E402
_FINDERS = [_StubFinder(own_only=True), _StubFinder(own_only=False)]
sys.meta_path.insert(0, _FINDERS[0])
sys.meta_path.append(_FINDERS[1])

cv2 = importlib.import_module("cv2")
assert isinstance(cv2, _StubModule), "a real cv2 is importable: bind nothing and record that the warp is cv2's"
MATRICES = []


def _warp_affine(src, m, dsize, *a, **k):
    MATRICES.append(np.array(m, np.float64))
    return otf.warp_affine(np.ascontiguousarray(src), m, dsize)


cv2.warpAffine = _warp_affine

from src.keypoints.datasets.coco import HeatmapGenerator, JointsGenerator, collate_fn  # noqa: E402
from src.keypoints.transforms import KeypointsTransform  # noqa: E402

for _f in _FINDERS:  # the stubs that exist stay in sys.modules; nothing new is stubbed from here on
    sys.meta_path.remove(_f)

OUT_SIZE, RESOLUTIONS, NUM_KPTS, SIGMA = 128, [1 / 4, 1 / 2], 17, 2
TRANSFORM = dict(max_rotation=30, min_scale=0.75, max_scale=1.5, scale_type="short", max_translate=40)
# (tag, mode, raw h, raw w, people, sample seed, RNG seed, mask holes)
CASES = [
    ("small_many", "train", 96, 80, 12, 1, 101, 2),
    ("large_one", "train", 200, 260, 1, 2, 102, 1),
    ("large_none", "train", 180, 150, 0, 3, 103, -1),
    ("tall_some", "train", 230, 110, 5, 4, 107, 2),
    ("long_side", "train_long", 120, 170, 4, 5, 108, 0),
    ("inference", "inference", 167, 224, 3, 6, 106, 1),
]
# the warped uint8 image is stored whole for these (noise does not compress); every case records its sha256, and a test that
# recomputes the image with oracle.transforms.warp_affine from the recorded matrix can check that hash first
FULL_IMAGES = ("small_many", "large_one")


def main():
    tf = {"train": KeypointsTransform(OUT_SIZE, RESOLUTIONS, **TRANSFORM),
          "train_long": KeypointsTransform(OUT_SIZE, RESOLUTIONS, **dict(TRANSFORM, scale_type="long"))}
    hm_sizes = [int(r * OUT_SIZE) for r in RESOLUTIONS]
    hm_gen = [HeatmapGenerator(NUM_KPTS, s, sigma=SIGMA) for s in hm_sizes]
    j_gen = [JointsGenerator(s) for s in hm_sizes]
    out, meta_cases, batch = {}, [], []
    for tag, mode, h, w, people, sseed, rseed, holes in CASES:
        img, mask, joints = synth.synth_train_sample(h, w, people, sseed, NUM_KPTS, holes)
        sha = hashlib.sha256(img.tobytes() + mask.tobytes() + joints.tobytes()).hexdigest()
        np.random.seed(rseed)
        random.seed(rseed)
        MATRICES.clear()
        pipeline = (tf["train"].inference if mode == "inference" else tf[mode].train).transforms
        steps = pipeline[:1] if mode == "inference" else pipeline[:2]  # RandomAffineTransform (+ RandomHorizontalFlip); not ToTensor / Normalize
        image, mask_list, joints_list = img, [mask.copy() for _ in hm_sizes], [joints.copy() for _ in hm_sizes]
        with Recorder() as rec:
            for t in steps:
                image, mask_list, joints_list = t(image, mask_list, joints_list)
        assert len(MATRICES) == len(hm_sizes) + 1
        flipped = any(n == "random.random" and v < 0.5 for n, v in rec.draws)
        out[f"{tag}.mats"], out[f"{tag}.mat_image"] = np.stack(MATRICES[:-1]), MATRICES[-1]
        image = np.ascontiguousarray(image)
        if tag in FULL_IMAGES:
            out[f"{tag}.image_u8"] = image
        heatmaps, leaving = [], 0
        for i in range(len(hm_sizes)):
            jf = np.array(joints_list[i], np.float64)
            # a last-ulp difference in a restated dot product must not be able to flip int(): no coordinate near an integer
            frac = np.abs(jf[..., :2] - np.round(jf[..., :2]))
            assert jf.size == 0 or frac.min() > 1e-6, f"{tag}: a transformed coordinate lies within 1e-6 of an integer; pick another seed"
            leaving += int(((jf[..., 2] > 0) & ((jf[..., 0] < 0) | (jf[..., 1] < 0) | (jf[..., 0] >= hm_sizes[i]) | (jf[..., 1] >= hm_sizes[i]))).sum())
            out[f"{tag}.joints_f{i}"] = jf
            joints_list[i] = j_gen[i](joints_list[i])
            out[f"{tag}.joints_i{i}"] = joints_list[i]
            heatmaps.append(hm_gen[i](joints_list[i]).astype(np.float32))
            out[f"{tag}.mask{i}"] = (mask_list[i] > 0).astype(np.uint8)
            assert set(np.unique(mask_list[i])) <= {0.0, 1.0} and mask_list[i].dtype == np.float32
        batch.append((image, heatmaps, mask_list, joints_list))
        meta_cases.append(dict(tag=tag, mode=mode, h=h, w=w, people=people, sample_seed=sseed, rng_seed=rseed, holes=holes, sha256=sha,
                               draws=rec.draws, flip=bool(flipped), image_sha256=hashlib.sha256(image.tobytes()).hexdigest(), joints_leaving_the_map=leaving,
                               people_per_stage=[int(len(j)) for j in joints_list]))
        print(tag, "flip", flipped, "draws", len(rec.draws), "people per stage", [len(j) for j in joints_list], "leaving", leaving)
    # collate_fn (coco.py:140-164) stacks the batch; the heatmaps are stored from its tensors
    images, hms, masks, joints = collate_fn(batch)
    for b, (tag, *_rest) in enumerate(CASES):
        for i in range(len(hm_sizes)):
            out[f"{tag}.hm{i}"] = hms[i][b].numpy()
            assert np.array_equal(masks[i][b].numpy() > 0, out[f"{tag}.mask{i}"] > 0) and np.array_equal(joints[i][b], out[f"{tag}.joints_i{i}"])
        assert hashlib.sha256(images[b].numpy().tobytes()).hexdigest() == meta_cases[b]["image_sha256"]
    train = [c for c in meta_cases if c["mode"] != "inference"]
    assert {c["flip"] for c in train} == {True, False}, "both flip outcomes are needed; pick other seeds"
    assert any(c["joints_leaving_the_map"] for c in meta_cases)
    os.makedirs(OUT, exist_ok=True)
    np.savez_compressed(os.path.join(OUT, "train_input.npz"), **out)
    meta = dict(out_size=OUT_SIZE, hm_resolutions=RESOLUTIONS, num_kpts=NUM_KPTS, sigma=SIGMA, transform=TRANSFORM, cases=meta_cases,
                warp="cv2.warpAffine was bound to oracle.transforms.warp_affine (the project's restatement of OpenCV 4.9's 8-bit "
                     "INTER_LINEAR warp): parity of the warped pixels with cv2 is UNPINNED; draws, matrices, joints, mask threshold, flip, "
                     "JointsGenerator, HeatmapGenerator and collate_fn are the reference's own code",
                raw_inputs="synth.synth_train_sample(h, w, people, sample_seed, num_kpts, holes); sha256 over image, mask, joints bytes")
    with open(os.path.join(OUT, "train_input_meta.json"), "w") as f:
        json.dump(meta, f, indent=1)
    print("wrote", os.path.getsize(os.path.join(OUT, "train_input.npz")), "bytes")


if __name__ == "__main__":
    main()
