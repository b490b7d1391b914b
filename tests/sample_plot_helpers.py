"""Shared by tests/test_sample_plot_cpu.py and tests/test_gpu_sample_plot.py: the overlay case list (frames sized around the kernel's
real tile, read from hh_seg_overlay_config) and the golden's loader."""
import importlib
import json
import os

import numpy as np
import pytest

import seg_overlay_ref as sr
from conftest import GOLDEN, PKG


@pytest.fixture(scope="session")
def sp():
    return importlib.import_module(PKG + ".keypoints.sample_plot")


@pytest.fixture(scope="session")
def sample_golden():
    meta = json.load(open(os.path.join(GOLDEN, "sample_plot_meta.json")))
    data = np.load(os.path.join(GOLDEN, "sample_plot.npz"))
    return meta, data


def obj(*polys, kpts=None):
    return {"segmentation": [list(map(float, np.asarray(p).reshape(-1))) for p in polys], "keypoints": kpts or [0] * 51, "iscrowd": 0,
            "num_keypoints": 0}


def rle_obj(mask: np.ndarray):
    """A run-length (iscrowd) object from a bool [h,w] mask: column-major runs, starting with a run of zeros."""
    flat = np.asarray(mask, bool).T.reshape(-1)
    bounds = np.concatenate([[0], np.flatnonzero(flat[1:] != flat[:-1]) + 1, [flat.size]])
    counts = ([0] if flat[0] else []) + np.diff(bounds).tolist()
    assert sum(counts) == flat.size
    return {"segmentation": {"size": list(mask.shape), "counts": counts}, "keypoints": [0] * 51, "iscrowd": 1, "num_keypoints": 0}


def _line(colour, xa, ya, xb, yb):
    return [sr.LINE, colour, xa, ya, xb, yb, 0, 0]


def overlay_cases(sp) -> list:
    """[(name, image uint8 [h,w,3], shapes int32 [n,8], toggles uint32, alpha, bgr)]: the frames and shapes the issue lists."""
    Th, Tw, _, chunk = sp.overlay_config()
    rng = np.random.default_rng(20240607)
    img = lambda h, w: rng.integers(0, 256, (h, w, 3), dtype=np.uint8)  # noqa: E731
    cases = []

    def add(name, h, w, annot=(), extra=(), alpha=0.4, bgr=False):
        shapes, toggles = sp.seg_tables(list(annot), h, w)
        if len(extra):
            shapes = np.concatenate([shapes, np.array(extra, np.int32).reshape(-1, 8)])
        cases.append((name, img(h, w), shapes, toggles, alpha, bgr))

    def blob(h, w, k):
        return sr.star_polygon(rng, h, w)[:max(k, 3)]

    add("one_pixel", 1, 1, [obj([0, 0, 0, 0, 0, 0])], [_line(0x0000FF, 0, 0, 0, 0)])
    add("one_pixel_blend_only", 1, 1)
    add("crosses_tiles_45x300", 45, 300, [obj(blob(45, 300, 9)), obj([5, 5, 290, 8, 280, 40, 140, 20, 10, 43]), obj(blob(45, 300, 5))])
    add("narrow_64x37", 64, 37, [obj(blob(64, 37, 7), blob(64, 37, 4)), obj([0, 0, 36, 0, 36, 63, 0, 63])])
    add("tile_plus_one", Th + 1, Tw + 1, [obj(blob(Th + 1, Tw + 1, 8)), obj([Tw - 2, Th - 2, Tw + 3, Th - 2, Tw + 3, Th + 4, Tw - 2, Th + 4])])
    add("two_tiles_and_a_bit", 2 * Th + 3, 2 * Tw + 5, [obj(blob(2 * Th + 3, 2 * Tw + 5, 12)) for _ in range(4)])
    add("no_shapes", 33, 70)
    add("no_shapes_alpha_1", 9, 5, alpha=1.0)
    add("outside", 40, 50,
        [obj([-20, -20, 30, -10, 25, 30, -15, 20]),            # partly outside, negative vertices
         obj([100, 100, 140, 100, 120, 150]),                   # wholly outside: an empty fill and lines that draw nothing
         obj([-30, 10, -5, 12, -10, 35]),                       # wholly left of the frame
         obj([30, 20, 90, 25, 60, 70])],                        # partly beyond right and bottom
        [_line(0x102030, -1000, -700, 2000, 1500), _line(0x405060, 49, -5, 49, 500), _line(0xA0B0C0, -(1 << 23), 39, 1 << 23, 39),
         _line(0x00FF00, 200, 200, 300, 300)])
    add("last_wins", 48, 140, [obj([10, 5, 120, 5, 120, 40, 10, 40]), obj([40, 0, 100, 0, 100, 47, 40, 47]), obj([60, 10, 135, 20, 70, 44])])
    # more rows than one chunk: a big fill first, chunk + 40 lines over it, then a fill that must end up on top of them all
    many = [_line(int(rng.integers(0, 1 << 24)), *(int(v) for v in rng.integers(-10, 150, 4))) for _ in range(chunk + 40)]
    late, late_t = sp.seg_tables([obj([20, 10, 110, 12, 100, 60, 30, 55])], 70, 140, palette=[(1, 2, 3)])
    first, first_t = sp.seg_tables([obj([2, 2, 137, 2, 137, 67, 2, 67])], 70, 140)
    late[late[:, 0] == sr.FILL, 2] += len(first_t)
    cases.append(("chunks", img(70, 140), np.concatenate([first, np.array(many, np.int32), late]), np.concatenate([first_t, late_t]), 0.4, False))
    disc = (np.hypot(*np.mgrid[-20:25, -30:40]) < 17) | (np.mgrid[0:45, 0:70][1] % 13 == 0)
    add("rle", 45, 70, [obj([3, 3, 60, 10, 30, 40]), rle_obj(disc)])
    add("degenerate", 30, 41,
        [obj([7, 7]), obj([3, 20, 35, 4]), obj([10, 10, 10, 10, 10, 10]), obj([5, 5, 30, 5, 30, 5, 30, 25, 5, 25, 5, 25]),
         obj([20, 2, 20, 28, 20, 15]), obj([1.9, -0.9, 38.7, 1.2, 20.5, 27.99])])
    add("bgr", 37, 131, [obj(blob(37, 131, 10)), obj(blob(37, 131, 6))], alpha=0.4, bgr=True)
    add("alpha_0", 20, 33, [obj(blob(20, 33, 6))], alpha=0.0)
    add("alpha_065", 20, 33, [obj(blob(20, 33, 6))], alpha=0.65)
    return cases


def reference(case):
    _, image, shapes, toggles, alpha, bgr = case
    w0, w1 = np.float32(1.0 - float(alpha)), np.float32(float(alpha))
    return sr.overlay(image, shapes, toggles, w0, w1, bgr)


# ---------------------------------------------------------------------------------------------------------------- the golden's inputs
OUT_SIZE, STAGE_SIZES, MEAN, STD = 128, (32, 64), (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def _kpts(rng, h, w, hidden=()):
    k = np.zeros((17, 3))
    k[:, 0], k[:, 1], k[:, 2] = rng.uniform(0.1 * w, 0.9 * w, 17), rng.uniform(0.1 * h, 0.9 * h, 17), 2
    k[list(hidden)] = 0
    return np.round(k, 1).reshape(-1).tolist()


def golden_items() -> list:
    """[(raw image uint8 [h,w,3], annotation, (img float32 [3,S,S], [heatmaps [17,s,s]], [mask [s,s]], [int32 joints [P,17,3]]), file
    stem)]: out_size 128 (stages 32 and 64), two raw images of different aspect, polygon objects only; one object has two polygons,
    one has no keypoints.  Everything is made here from seeds, so the golden files hold recorded results only."""
    import text_ref
    rng = np.random.default_rng(77)
    items = []
    for n, (h, w, stem) in enumerate(((90, 140, "000000000139"), (120, 80, "000000000785"))):
        raw = text_ref.image(40 + n, h, w)
        if n == 0:
            annot = [dict(obj([20.7, 10.2, 70.1, 14.9, 60.5, 70.3, 25.0, 64.6], kpts=_kpts(rng, h, w, hidden=(3, 4))), num_keypoints=15),
                     dict(obj([80.2, 20.8, 130.9, 25.1, 125.4, 50.0], [90.0, 55.5, 135.2, 60.1, 120.7, 88.9, 85.3, 80.0], kpts=_kpts(rng, h, w)), num_keypoints=17),
                     obj([5.5, 60.5, 40.2, 62.0, 30.9, 86.1])]   # no keypoints
        else:
            annot = [dict(obj([10.1, 15.9, 70.6, 20.2, 65.0, 110.4, 12.8, 100.7], kpts=_kpts(rng, h, w, hidden=(0, 15, 16))), num_keypoints=14),
                     dict(obj([30.3, 40.4, 75.5, 45.6, 50.7, 95.8], kpts=_kpts(rng, h, w, hidden=range(5, 17))), num_keypoints=5)]
        img = ((text_ref.image(50 + n, OUT_SIZE, OUT_SIZE).astype(np.float32) / 255 - np.array(MEAN, np.float32)) / np.array(STD, np.float32)).transpose(2, 0, 1)
        people = np.array([o["keypoints"] for o in annot if o["iscrowd"] == 0 and o["num_keypoints"] > 0]).reshape(-1, 17, 3)
        heatmaps, masks, joints_list = [], [], []
        for s in STAGE_SIZES:
            j = np.zeros(people.shape, np.int32)
            j[..., 0], j[..., 1], j[..., 2] = people[..., 0] * s / w, people[..., 1] * s / h, people[..., 2] > 0
            yy, xx = np.mgrid[0:s, 0:s].astype(np.float32)
            hm = np.zeros((17, s, s), np.float32)
            for person in j:
                for k, (x, y, v) in enumerate(person):
                    if v:
                        hm[k] = np.maximum(hm[k], np.exp(-((xx - x) ** 2 + (yy - y) ** 2) / 8).astype(np.float32))
            mask = np.ones((s, s), np.float32)
            mask[s // 8:s // 3, s // 2:s - 3] = 0
            heatmaps.append(hm), masks.append(mask), joints_list.append(j)
        items.append((raw, annot, (np.ascontiguousarray(img), heatmaps, masks, joints_list), stem))
    return items
