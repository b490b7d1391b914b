#!/usr/bin/env python3
"""Fill and contour of the segmentation overlay against Pillow's ImageDraw.polygon(fill, outline), on the 300 seeded star polygons of
tests/test_sample_plot_cpu.py::test_fill_and_contour_leave_no_seam (the same seed and generator, tests/seg_overlay_ref.star_polygon).

  python3 tools/seg_overlay_vs_pillow.py

Runs on the CPU (the tables come from keypoints/sample_plot.seg_tables, the coverage from the numpy restatement of the rule); needs the
built library for the polygon toggles, no GPU.  Information for profiles/sample_plot.md, not an assertion: Pillow is not cv2 either.
Prints one JSON line."""
import importlib
import json
import os
import sys

import numpy as np
from PIL import Image, ImageDraw, __version__ as pillow_version

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import seg_overlay_ref as sr  # noqa: E402

sp = importlib.import_module("pytorch-human-pose_amd.keypoints.sample_plot")


def polygon_object(poly):
    return {"segmentation": [[float(v) for v in np.asarray(poly).reshape(-1)]], "keypoints": [0] * 51, "iscrowd": 0, "num_keypoints": 0}


def main():
    rng = np.random.default_rng(300)
    res = dict(pillow=pillow_version, polygons=300, pillow_pixels=0, differing=0, worst_polygon=0, here_only=0, pillow_only=0, strictly_inside=0,
               uncovered=0, uncovered_without_shift=0)
    for _ in range(res["polygons"]):
        h, w = int(rng.integers(20, 91)), int(rng.integers(20, 121))
        poly = sr.star_polygon(rng, h, w)
        mine = sr.covered(*sp.seg_tables([polygon_object(poly)], h, w), h, w)
        unshifted = sr.covered(*sp.seg_tables([polygon_object(poly)], h, w, shift=0.0), h, w)
        canvas = Image.new("L", (w, h), 0)
        ImageDraw.Draw(canvas).polygon([tuple(int(v) for v in p) for p in poly], fill=255, outline=255)
        pil = np.asarray(canvas) > 0
        inside = sr.strictly_inside(poly, h, w)
        differ = int((mine ^ pil).sum())
        res["pillow_pixels"] += int(pil.sum())
        res["differing"] += differ
        res["worst_polygon"] = max(res["worst_polygon"], differ)
        res["here_only"] += int((mine & ~pil).sum())
        res["pillow_only"] += int((pil & ~mine).sum())
        res["strictly_inside"] += int(inside.sum())
        res["uncovered"] += int((inside & ~mine).sum())
        res["uncovered_without_shift"] += int((inside & ~unshifted).sum())
    print(json.dumps(res))


if __name__ == "__main__":
    main()
