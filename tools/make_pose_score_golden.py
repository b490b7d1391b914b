#!/usr/bin/env python3
"""Generate tests/golden/pose_score.npz + pose_score_meta.json by RUNNING the reference's match_preds_to_targets and
InferenceKeypointsResult.calculate_OKS (src/keypoints/results.py), object_OKS / image_OKS (src/keypoints/datasets/coco.py) and
object_PCKh / image_PCKh (src/keypoints/datasets/mpii.py) on the lattice of tests/pose_score_budget.py.

  PYTHONDONTWRITEBYTECODE=1 python3 tools/make_pose_score_golden.py [path to a checkout of the reference, default /root/reference] [output directory]

Needs a checkout of the reference (thawro/pytorch-human-pose) and this repository's built library (the lattice takes the COCO
variances and the head sizes from the package); nothing of the reference is copied: the fixture holds numbers only, inputs and outputs.

What runs is the reference's own code: the stable ascending walk, the strict-greater selection, the visibility mask, numpy's pairwise
sums and means, np.exp, round(3), the in-place reorder of calculate_OKS.  The predictions go in with the dtype a result holds them in
(float32; float64 for the fallback pseudo-person), the targets as the integers an annotation holds.  For PCKh the predictions go in as
float64: the header's rule is fp64 throughout.
What is NOT the reference's: cv2 is not installed where the fixtures are made, so cv2.contourArea is a stand-in that evaluates the
header's shoelace (tests/pose_score_ref.polygon_area) on the int32 array the reference hands it.  Parity of the polygon area with cv2
therefore stays UNPINNED (recorded in the meta file).
"""
import importlib
import json
import os
import sys
import types

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
if not os.path.isdir(os.path.join(REF, "src", "keypoints")):
    raise SystemExit(f"{REF} is no checkout of the reference\n" + __doc__)
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(REPO, "tests", "golden")
sys.dont_write_bytecode = True
sys.path.insert(0, REF)
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import torch  # noqa: E402,F401

import pose_score_budget as lat  # noqa: E402
import pose_score_ref  # noqa: E402


class _Anything(types.ModuleType):
    """A module whose every attribute is a do-nothing class (callable, and usable in an annotation such as `X | None`)."""
    __path__: list = []

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return type(name, (), {"__init__": lambda self, *a, **k: None})


try:
    importlib.import_module("cv2")
    raise SystemExit("a real cv2 is importable: use its contourArea and record that the polygon area is cv2's")
except ImportError:
    cv2 = sys.modules["cv2"] = _Anything("cv2")
AREA_CALLS = []


def _contour_area(contour):
    assert contour.dtype == np.int32 and contour.ndim == 2 and contour.shape[1] == 2
    AREA_CALLS.append(len(contour))
    return pose_score_ref.polygon_area(contour)


cv2.contourArea = _contour_area

# the packages' __init__ files pull in configuration code that is not needed here; neither are the logger, the model base and the loaders
for _pkg in ("src", "src.utils", "src.base", "src.base.datasets", "src.base.transforms", "src.keypoints", "src.keypoints.datasets"):
    m = types.ModuleType(_pkg)
    m.__path__ = [os.path.join(REF, *_pkg.split("."))]
    sys.modules[_pkg] = m
for _name, _attrs in (("src.logger", {}), ("src.logger.pylogger", {"log": None}), ("src.base.model", {"BaseInferenceModel": object}),
                      ("src.base.results", {"BaseResult": object}), ("src.utils.files", {"load_yaml": None, "save_yaml": None}),
                      ("src.utils.utils", {"get_rank": None}), ("pycocotools", {}), ("pycocotools.coco", {"COCO": object}), ("natsort", {})):
    m = types.ModuleType(_name)
    m.__dict__.update(_attrs)
    sys.modules[_name] = m
for _name in ("seaborn", "torchvision", "torchvision.transforms", "torchvision.transforms.functional", "albumentations", "matplotlib",
              "matplotlib.pyplot", "src.keypoints.grouping", "src.keypoints.transforms", "src.keypoints.visualization", "src.utils.image",
              "src.base.transforms.utils"):
    sys.modules.setdefault(_name, _Anything(_name))

try:
    base = importlib.import_module("src.base.datasets.base")
    sys.modules["src.base.datasets"].BaseImageDataset = base.BaseImageDataset
except Exception:  # noqa: BLE001  (only the scoring functions of coco.py are needed)
    sys.modules["src.base.datasets"].BaseImageDataset = object
coco = importlib.import_module("src.keypoints.datasets.coco")
mpii = importlib.import_module("src.keypoints.datasets.mpii")
results = importlib.import_module("src.keypoints.results")
REF_VARIANCES = coco.variances.copy()


def run_case(name):
    c, t, _ = lat.case(name)
    tg, K = t["targets"], c["K"]
    out = {"p_off": np.cumsum([0] + [len(s) for _, s in t["preds"]]).astype(np.int32), "p_xy": np.concatenate([xy for xy, _ in t["preds"]]),
           "p_score": np.concatenate([s for _, s in t["preds"]]), "t_off": tg["t_off"], "t_xyv": tg["t_xyv"], "t_head": tg["t_head"],
           "variances": np.asarray(c["variances"], np.float64)}
    match, obj, value, calc, area = [], [], [], [], []
    if c["metric"] == "oks":
        assert K != 17 or np.array_equal(REF_VARIANCES, c["variances"]), "the package's OKS_VARIANCES are not the reference's"
        coco.variances = np.asarray(c["variances"], np.float64)  # (K = 3: the case's own; the functions read the module's array)
    for b, im in enumerate(c["images"]):
        xy64, sc = t["preds"][b]
        dt = np.float64 if im["flag"] or c["metric"] == "pckh" else np.float32
        xy, sc = xy64.astype(dt), sc.astype(np.float64 if im["flag"] else np.float32)
        assert np.array_equal(xy.astype(np.float64), xy64)
        kp = im["t_xyv"].astype(np.int64)
        assert np.array_equal(kp, im["t_xyv"]), "annotations hold integers"
        T = len(kp)
        m = results.match_preds_to_targets(xy, sc, kp[..., :2], kp[..., 2]) if T else []
        match.append(np.asarray(m, np.int32))
        if c["metric"] == "oks":
            for j in range(T):
                before = len(AREA_CALLS)
                obj.append(coco.object_OKS(xy[m[j]], kp[j, :, :2], kp[j, :, 2], im["polygons"][j]))
                assert len(AREA_CALLS) - before == len(im["polygons"][j])
                area.append(pose_score_ref.object_area(im["polygons"][j]))
            value.append(coco.image_OKS(xy[m], kp[..., :2], kp[..., 2], im["polygons"]) if T else -1)
            annot = [{"keypoints": kp[j].reshape(-1).tolist(), "segmentation": im["polygons"][j]} for j in range(T)]
            stub = types.SimpleNamespace(annot=annot, kpts_coords=xy.copy(), kpts_scores=np.zeros(xy.shape[:2], np.float32), obj_scores=sc.copy())
            calc.append(results.InferenceKeypointsResult.calculate_OKS(stub))
        else:
            for j in range(T):
                obj.append(mpii.object_PCKh(xy[m[j]], kp[j, :, :2], kp[j, :, 2], im["heads"][j], c["alpha"]))
                area.append(pose_score_ref.SPACING)
            value.append(mpii.image_PCKh(c["alpha"], xy[m], kp[..., :2], kp[..., 2], im["heads"]) if T else -1)
    out.update(match=np.concatenate(match), obj=np.asarray(obj, np.float64), value=np.asarray(value, np.float64), t_area=np.asarray(area, np.float64))
    if calc:
        out["calculate_OKS"] = np.asarray(calc, np.float64)
    return c, out


def main():
    arrays, meta = {}, {"cases": {}, "reference_functions": ["match_preds_to_targets", "object_OKS", "image_OKS", "calculate_OKS", "object_PCKh", "image_PCKh"],
                        "UNPINNED": "cv2.contourArea is a stand-in evaluating the header's int64 shoelace: cv2 is absent where the fixture is made",
                        "numpy": np.__version__}
    for name in lat.LATTICE:
        c, out = run_case(name)
        for k, v in out.items():
            arrays[f"{name}/{k}"] = v
        meta["cases"][name] = {"seed": int(c["seed"]), "K": int(c["K"]), "metric": c["metric"], "alpha": float(c["alpha"]), "images": len(c["images"]),
                               "targets": int(out["t_off"][-1]), "predictions": int(out["p_off"][-1])}
    meta["contourArea_calls"] = len(AREA_CALLS)
    np.savez_compressed(os.path.join(OUT, "pose_score.npz"), **arrays)
    with open(os.path.join(OUT, "pose_score_meta.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(meta["cases"]), os.path.getsize(os.path.join(OUT, "pose_score.npz")), "bytes")


if __name__ == "__main__":
    main()
