#!/usr/bin/env python3
"""Generate tests/golden/render.npz + render_meta.json by RUNNING the reference's plot_connections (src/keypoints/visualization.py) on
seeded and hand-placed poses.

  PYTHONDONTWRITEBYTECODE=1 python3 tools/make_render_golden.py <path to a checkout of the reference>

Needs a checkout of the reference (thawro/pytorch-human-pose); nothing of it is copied: the fixture holds arrays and numbers only.

What is imported from the reference and therefore pinned by the fixture: plot_connections and draw_elipsis (which primitives, in what
order, where, how large, which colour, the thresholds, the truncations, the floor division of the limb centre, the axis branches, the
angle, the blend weights) and utils/image.py's get_color (recorded for i in 0..99).
What is NOT the reference's: cv2 and seaborn are not installed where the fixtures are made.  Both are replaced by empty stand-in
modules; cv2.ellipse, cv2.circle and cv2.addWeighted are bound to the recorders of tests/render_ref.py, which log every call and
rasterise it by the rule stated in include/hhrnet.h.  Parity of the covered pixel set with cv2's own rasteriser therefore stays
UNPINNED.
"""
import importlib
import json
import os
import sys
import types

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if len(sys.argv) < 2:
    raise SystemExit(__doc__)
REF = sys.argv[1]
sys.dont_write_bytecode = True
sys.path.insert(0, REF)
sys.path.insert(0, os.path.join(REPO, "tests"))
OUT = os.path.join(REPO, "tests", "golden")

import render_ref  # noqa: E402


class _Anything(types.ModuleType):
    """A module whose every attribute is a do-nothing callable (seaborn.set_style at import time, cv2's constants)."""
    __path__: list = []

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return lambda *a, **k: None


for _name in ("cv2", "seaborn"):
    try:
        importlib.import_module(_name)
        raise SystemExit(f"a real {_name} is importable: bind nothing and record that the rasteriser is cv2's")
    except ImportError:
        sys.modules[_name] = _Anything(_name)
if "src.utils" not in sys.modules:  # the packages' __init__ files pull in configuration code that is not needed here
    for _pkg in ("src", "src.utils", "src.keypoints"):
        m = types.ModuleType(_pkg)
        m.__path__ = [os.path.join(REF, *_pkg.split("."))]
        sys.modules[_pkg] = m

cv2 = sys.modules["cv2"]
vis = importlib.import_module("src.keypoints.visualization")
get_color = importlib.import_module("src.utils.image").get_color

K, LIMBS = 17, render_ref.COCO_LIMBS
H, W = 96, 128
THR = 0.25  # exact in binary: "a score equal to thr" means the same in every float format


def image(seed, h=H, w=W):
    """A seeded frame of 4 x 4 blocks (it compresses well; the blend still meets many byte values)."""
    blocks = np.random.default_rng(seed).integers(0, 256, ((h + 3) // 4, (w + 3) // 4, 3), dtype=np.uint8)
    return np.ascontiguousarray(np.repeat(np.repeat(blocks, 4, 0), 4, 1)[:h, :w])


def people(seed, P, h=H, w=W, spread=30.0):
    """P seeded people: a centre inside the frame, keypoints scattered around it, fractional coordinates, scores in (thr, 1) with a
    few below thr."""
    rng = np.random.default_rng(seed)
    centre = rng.uniform([10, 10], [w - 10, h - 10], (P, 1, 2))
    coords = centre + rng.normal(0, spread / 2, (P, K, 2))
    scores = rng.uniform(0.3, 1.0, (P, K))
    scores[rng.uniform(size=(P, K)) < 0.15] = 0.1
    return coords, scores


def edge_people():
    """Four hand-placed people (x, y); the limb indices refer to COCO_LIMBS."""
    coords = np.zeros((4, K, 2))
    scores = np.full((4, K), 0.9)
    # person 0: the threshold.  Keypoint 0 scores exactly thr (drawn, and so are its limbs), keypoint 1 just below (not drawn)
    coords[0] = people(71, 1)[0][0]
    scores[0, 0], scores[0, 1] = THR, np.nextafter(THR, 0)
    # person 1: every score below thr: nothing of it is drawn, but it still takes palette index 1
    coords[1] = people(72, 1)[0][0]
    scores[1] = 0.2
    # person 2: hand-placed limbs
    p = coords[2]
    p[15], p[13] = (40.2, 30.7), (40.9, 30.1)          # limb 0: both ends on pixel (40, 30)
    p[11] = (52.5, 42.5)                               # limb 1 (13 -> 11): dx = dy = 12, |dx| == |dy|: the second branch
    p[16], p[14] = (-5.0, 10.0), (2.0, 20.0)           # limb 2: x1 + x2 = -3: floor -2, truncation -1; partly left of the frame
    p[12] = (30.0, 20.0)                               # limb 3 (14 -> 12): axis-aligned, horizontal; limb 4 (11 -> 12): dx < 0, dy < 0
    p[5], p[6] = (70.999999999, 60.999999999), (52.0, 90.0)  # fractional just below an integer; limb 5 (5 -> 11): dx < 0, dy < 0, |dx| > |dy|
    p[7], p[8] = (70.0, 80.0), (140.0, 100.0)          # limb 8 (5 -> 7): vertical; limb 9 (6 -> 8): dx > 0, dy > 0, runs beyond the right edge
    p[9], p[10] = (90.0, 70.0), (120.0, 110.0)         # limb 10 (7 -> 9): dx > 0, dy < 0; limb 11 (8 -> 10): dx < 0, dy > 0, below the frame
    p[1], p[2], p[0] = (100.0, 20.0), (110.0, 10.0), (105.0, -7.5)   # limb 12: dx > 0, dy < 0 with |dx| == |dy|; limbs 13, 14 above the frame
    p[3], p[4] = (-20.5, -3.5), (125.0, 30.0)          # a keypoint wholly outside; int(-20.5) = -20, int(-3.5) = -3
    # person 3: tall enough for s = 3 (y range 330 -> int(3.3)); the keypoint that makes it so tall is below thr and far outside
    coords[3] = people(73, 1, spread=16.0)[0][0]
    coords[3, 16] = (60.0, coords[3, :16, 1].min() + 330.0)
    scores[3] = 0.9
    scores[3, 16] = 0.1
    return coords, scores


# (tag, frame seed, people, colour mode, alpha)
CASES = [
    ("person_a08", 1, people(11, 3), "person", 0.8),
    ("limb_a065", 2, people(12, 3), "limb", 0.65),
    ("one_a0", 3, people(13, 1), "person", 0.0),
    ("one_a1", 4, people(14, 1), "limb", 1.0),
    ("nobody", 5, (np.zeros((0, K, 2)), np.zeros((0, K))), "person", 0.8),
    ("crowd30", 6, people(15, 30), "person", 0.8),
    ("edges_person", 7, edge_people(), "person", 0.8),
    ("edges_limb", 7, edge_people(), "limb", 0.65),
]


def main():
    out, meta_cases = {}, []
    palette = np.stack([get_color(i) for i in range(100)])
    assert palette.dtype == np.uint8 and palette.shape == (100, 3)
    out["get_color"] = palette
    for tag, seed, (coords, scores), mode, alpha in CASES:
        img = image(seed)
        before = img.copy()
        rec = render_ref.Recorder()
        cv2.ellipse, cv2.circle, cv2.addWeighted = rec.ellipse, rec.circle, rec.addWeighted
        got = vis.plot_connections(img, coords, scores, LIMBS, thr=THR, color_mode=mode, alpha=alpha)
        assert np.array_equal(img, before), "the reference modified its input"
        # the stand-in rasterised with cos / sin of the logged angle; the rule forms c, s from sqrt and a division: same fp32 values,
        # same pixels, or the fixture would pin a libm
        ruled = render_ref.render(img, coords, scores, LIMBS, THR, mode, alpha, palette)
        assert np.array_equal(got, ruled), f"{tag}: cos / sin of the angle and the rule's direction differ in fp32"
        calls = rec.rows()
        out[f"{tag}.image"], out[f"{tag}.coords"], out[f"{tag}.scores"] = img, coords, scores
        out[f"{tag}.calls"], out[f"{tag}.out"] = calls, got
        meta_cases.append(dict(tag=tag, frame_seed=seed, people=int(len(coords)), color_mode=mode, alpha=alpha, thr=THR, calls=int(len(calls)),
                               changed_pixels=int((got != img).any(-1).sum())))
        print(tag, "people", len(coords), "calls", len(calls), "changed pixels", meta_cases[-1]["changed_pixels"])
    np.savez_compressed(os.path.join(OUT, "render.npz"), **out)
    meta = dict(num_kpts=K, limbs=[list(l) for l in LIMBS], thr=THR, frame=[H, W], cases=meta_cases,
                call_row="float64 [N,10]: (0 ellipse | 1 circle | 2 addWeighted, cx, cy, a or radius, b or radius, angle in degrees, r, g, b, "
                         "thickness); the addWeighted row is (2, w0, w1, 0...) with the doubles the reference passed",
                rasteriser="cv2.ellipse, cv2.circle and cv2.addWeighted were bound to tests/render_ref.Recorder (the project's stated rule, "
                           "include/hhrnet.h at hh_render_poses_u8_batch): parity of the covered pixels with cv2 is UNPINNED; which "
                           "primitives, their order, centres, axes, angles, colours, the thresholds, truncations and blend weights are the "
                           "reference's own code; get_color is the reference's get_color(i) for i in 0..99")
    with open(os.path.join(OUT, "render_meta.json"), "w") as f:
        json.dump(meta, f, indent=1)
    print("wrote", os.path.getsize(os.path.join(OUT, "render.npz")), "bytes")


if __name__ == "__main__":
    main()
