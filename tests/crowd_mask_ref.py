"""The crowd-mask rule of include/hhrnet.h (hh_crowd_polygon_toggles / hh_crowd_masks_u8_batch) restated in numpy from the header's
text.  It does NOT call the library: the tests compare the library and the kernel against it.

A segment (one polygon or one run-length list of an h x w image) reduces to a toggle list: strictly increasing uint32 positions in
0 .. h*w.  Pixels are numbered column-major, idx = x*h + y; a pixel is covered by the segment iff the number of toggles <= idx is odd;
a mask byte is 0 where at least one segment covers the pixel (a union, not XOR) and 255 elsewhere.  Parity of the polygon conversion
and of the list-of-lists dispatch with the COCO API itself is UNPINNED: the header's text is the contract."""
import math

import numpy as np


def cancel(positions) -> np.ndarray:
    """Sorted, values of even multiplicity dropped, values of odd multiplicity kept once -> uint32."""
    values, counts = np.unique(np.asarray(positions, np.int64), return_counts=True)
    return values[counts % 2 == 1].astype(np.uint32)


def _trunc(v: float) -> int:
    return int(v)  # Python's int() of a float truncates toward zero, as the C conversion does


def polygon_points(xy):
    """Steps 1 and 2: the dense point list (u, v) over all edges, on the five-fold grid."""
    xy = [float(v) for v in xy]
    k = len(xy) // 2
    X = [_trunc(5 * xy[2 * j] + 0.5) for j in range(k)]
    Y = [_trunc(5 * xy[2 * j + 1] + 0.5) for j in range(k)]
    X.append(X[0])
    Y.append(Y[0])
    pts = []
    for j in range(k):
        dx, dy = abs(X[j + 1] - X[j]), abs(Y[j + 1] - Y[j])
        flipped = (dx >= dy and X[j] > X[j + 1]) or (dx < dy and Y[j] > Y[j + 1])
        xs, ys, xe, ye = (X[j + 1], Y[j + 1], X[j], Y[j]) if flipped else (X[j], Y[j], X[j + 1], Y[j + 1])
        if dx == 0 and dy == 0:
            pts.append((X[j], Y[j]))
        elif dx >= dy:
            s = float(ye - ys) / dx
            for d in range(dx + 1):
                t = dx - d if flipped else d
                pts.append((xs + t, _trunc(ys + s * t + 0.5)))
        else:
            s = float(xe - xs) / dy
            for d in range(dy + 1):
                t = dy - d if flipped else d
                pts.append((_trunc(xs + s * t + 0.5), ys + t))
    return pts


def polygon_positions(xy, h: int, w: int) -> list:
    """Step 3: the emitted positions, before sorting and cancelling."""
    pts = polygon_points(xy)
    out = []
    for i in range(1, len(pts)):
        (u, v), (pu, pv) = pts[i], pts[i - 1]
        if u == pu:
            continue
        xd = float(u if u < pu else u - 1)
        xd = (xd + 0.5) / 5 - 0.5
        if math.floor(xd) != xd or xd < 0 or xd > w - 1:
            continue
        yd = float(min(v, pv))
        yd = (yd + 0.5) / 5 - 0.5
        yd = math.ceil(min(max(yd, 0.0), float(h)))
        out.append(int(xd) * h + int(yd))
    return out


def polygon_toggles(xy, h: int, w: int) -> np.ndarray:
    if len(xy) % 2 or len(xy) < 6:
        raise ValueError("a polygon needs an even count of at least 6 numbers")
    return cancel(polygon_positions(xy, h, w))


def rle_toggles(counts, h: int, w: int) -> np.ndarray:
    if isinstance(counts, (str, bytes)):
        raise ValueError("compressed run-length strings are not supported")
    counts = [int(c) for c in counts]
    if any(c < 0 for c in counts) or sum(counts) != h * w:
        raise ValueError("run lengths must be non-negative and sum to h*w")
    return cancel(np.cumsum(counts)[:-1])


def covered(toggles, h: int, w: int) -> np.ndarray:
    """bool [h,w]: the pixels one segment covers."""
    idx = np.arange(w, dtype=np.int64)[None, :] * h + np.arange(h, dtype=np.int64)[:, None]
    return (np.searchsorted(np.asarray(toggles, np.int64), idx, side="right") & 1).astype(bool)


def mask_from_toggles(toggle_lists, h: int, w: int) -> np.ndarray:
    """uint8 [h,w]: 0 where at least one segment covers the pixel, 255 elsewhere."""
    cov = np.zeros((h, w), bool)
    for t in toggle_lists:
        cov |= covered(t, h, w)
    return np.where(cov, 0, 255).astype(np.uint8)


def segment_toggles(segmentation, h: int, w: int) -> list:
    """One object's segmentation -> its toggle lists, by the dispatch of the header."""
    if isinstance(segmentation, dict):
        if [int(v) for v in segmentation["size"]] != [h, w]:
            raise ValueError("run-length size differs from the image")
        return [rle_toggles(segmentation["counts"], h, w)]
    entries = [list(e) for e in segmentation]
    if entries and len(entries[0]) == 4:
        out = []
        for e in entries:
            if len(e) != 4:
                raise ValueError("a box needs 4 numbers")
            x, y, bw, bh = e
            out.append(polygon_toggles([x, y, x, y + bh, x + bw, y + bh, x + bw, y], h, w))
        return out
    return [polygon_toggles(e, h, w) for e in entries]


def annotation_toggles(annot, h: int, w: int) -> list:
    out = []
    for obj in annot:
        if obj["iscrowd"] or obj["num_keypoints"] == 0:
            out.extend(segment_toggles(obj["segmentation"], h, w))
    return out


def crowd_mask_reference(annot, h: int, w: int) -> np.ndarray:
    """bool [h,w], True where no contributing object covers the pixel: get_crowd_mask of the reference's dataset under the rule above."""
    return mask_from_toggles(annotation_toggles(annot, h, w), h, w) == 255
