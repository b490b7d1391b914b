"""Shared by tests/test_crowd_mask_cpu.py and tests/test_gpu_crowd_mask.py: the fixtures of the rule as stated with it (h = 8, w = 9,
rows top to bottom, '1' = covered), the seeded polygon lattice, and the staging of one mask's tables for the library's host walk."""
import ctypes as C

import numpy as np
import pytest

import crowd_mask_ref as ref

H8, W9 = 8, 9
RECTANGLE = [0, 0, 0, 4, 4, 4, 4, 0]
TRIANGLE = [1.5, 1.2, 7.3, 2.0, 4.1, 9.7]
BOW_TIE = [1, 1, 7, 7, 7, 1, 1, 7]
OFF_RIGHT = [5, 2, 15, 2, 15, 6, 5, 6]
OFF_BOTTOM = [2, 5, 6, 5, 6, 12, 2, 12]
OFF_LEFT = [-5, 2, 3, 2, 3, 6, -5, 6]
OFF_TOP = [2, -6, 6, -6, 6, 3, 2, 3]
OUTSIDE = [20, 20, 30, 20, 30, 30]
ZERO_AREA = [1, 3, 7, 3, 4, 3]


def box_rows(r0, r1, c0, c1, h=H8, w=W9):
    """The picture of a covered block of rows r0..r1 x columns c0..c1 (inclusive)."""
    return ["".join("1" if r0 <= r <= r1 and c0 <= c <= c1 else "0" for c in range(w)) for r in range(h)]


# (polygon, emitted positions or None, covered pixels, the picture)
FIXTURES = {
    "rectangle": (RECTANGLE, None, 16, box_rows(0, 3, 0, 3)),
    "triangle": (TRIANGLE, 10, 22, "000000000 / 001100000 / 001111100 / 001111100 / 000111000 / 000111000 / 000111000 / 000010000".split(" / ")),
    "bow_tie": (BOW_TIE, 12, 18, ["000000000"] + "010000100 / 011001100 / 011111100 / 011001100 / 010000100".split(" / ") + ["000000000"] * 2),
    "off_right": (OFF_RIGHT, None, 16, box_rows(2, 5, 5, 8)),
    "off_bottom": (OFF_BOTTOM, None, 12, box_rows(5, 7, 2, 5)),
    "off_left": (OFF_LEFT, None, 12, box_rows(2, 5, 0, 2)),
    "outside": (OUTSIDE, None, 0, box_rows(1, 0, 1, 0)),
    "zero_area": (ZERO_AREA, None, 0, box_rows(1, 0, 1, 0)),
}


def picture(covered) -> list:
    return ["".join("1" if v else "0" for v in row) for row in covered]


def lattice(count=400, seed=2024):
    """[(h, w, xy)]: `count` seeded random polygons of 3..8 vertices, h and w drawn from 1..71, coordinates uniform in
    [-4, side + 4]."""
    rng = np.random.RandomState(seed)
    out = []
    for _ in range(count):
        k, h, w = int(rng.randint(3, 9)), int(rng.randint(1, 72)), int(rng.randint(1, 72))
        xy = np.empty(2 * k)
        xy[0::2] = rng.uniform(-4, w + 4, k)
        xy[1::2] = rng.uniform(-4, h + 4, k)
        out.append((h, w, xy))
    return out


def column_range(t, h, w):
    """The inclusive column range a toggle list can cover, from the header's text: the first toggle's column through the column of
    the pixel before the last toggle, or through the last column for an odd count."""
    first = min(int(t[0]) // h, w - 1)
    return first, (w - 1 if len(t) % 2 else max((int(t[-1]) - 1) // h, first))


def stage_one(cm, toggle_lists, h, w, ranges=None):
    """One mask's tables in one host buffer, as the library wants them: -> (buffer, mask desc view, seg desc view)."""
    lists = [np.asarray(t, np.uint32) for t in toggle_lists]
    seg_at = cm.MASK_DESC.itemsize
    tog_at = seg_at + cm.SEG_DESC.itemsize * len(lists)
    buf = np.zeros(tog_at + 4 * sum(t.size for t in lists) + 8, np.uint8)
    md, sd = buf[:seg_at].view(cm.MASK_DESC), buf[seg_at:tog_at].view(cm.SEG_DESC)
    md[0] = (0, h, w, 0, len(lists))
    for s, t in enumerate(lists):
        rng = ranges[s] if ranges is not None else (column_range(t, h, w) if t.size else (0, 0))
        sd[s] = (tog_at, t.size, rng[0], rng[1], 0)
        buf[tog_at:tog_at + 4 * t.size].view(np.uint32)[:] = t
        tog_at += 4 * t.size
    return buf, md, sd


def host_walk(pkg, toggle_lists, h, w, ranges=None):
    """hh_debug_crowd_masks_host -> (rc, uint8 [h,w])."""
    cm = pkg.keypoints.crowd_mask
    buf, md, sd = stage_one(cm, toggle_lists, h, w, ranges)
    out = np.full((h, w), 7, np.uint8)
    rc = pkg._lib.load().hh_debug_crowd_masks_host(out.ctypes.data, md.ctypes.data, sd.ctypes.data if len(sd) else None, buf.ctypes.data, len(sd))
    return rc, out


def person(iscrowd, num_keypoints, segmentation, seed=0, num_kpts=17):
    """One COCO object."""
    rng = np.random.RandomState(seed)
    kp = rng.randint(0, 40, (num_kpts, 3))
    kp[:, 2] = rng.randint(0, 3, num_kpts)
    return {"iscrowd": iscrowd, "num_keypoints": num_keypoints, "segmentation": segmentation, "keypoints": kp.reshape(-1).tolist()}


@pytest.fixture(scope="module")
def cm(pkg):
    return pkg.keypoints.crowd_mask
