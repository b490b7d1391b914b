"""The segmentation overlay's rule (hh_seg_overlay_u8_batch in include/hhrnet.h) restated in numpy and Python integers, independently
of the C code: the fill predicate on column-major toggles, the line rule with floor division, the draw order (the last row that covers a
pixel wins) and the fp32 blend over every pixel.  Shapes are the int32 rows {kind, colour, a, b, c, d, 0, 0} of the header."""
from fractions import Fraction

import numpy as np

FILL, LINE = 0, 1


def fill_mask(toggles, h: int, w: int) -> np.ndarray:
    """bool [h,w]: pixel (x, y) is covered iff the number of toggles <= x*h + y is odd."""
    y, x = np.mgrid[0:h, 0:w]
    return np.searchsorted(np.asarray(toggles, np.int64), x.astype(np.int64) * h + y, side="right") % 2 == 1


def line_pixels(xa: int, ya: int, xb: int, yb: int) -> list:
    """The pixels (x, y) of one line by the stated rule, in Python integers (// is floor division)."""
    xa, ya, xb, yb = int(xa), int(ya), int(xb), int(yb)
    dx, dy = abs(xb - xa), abs(yb - ya)
    if dx == 0 and dy == 0:
        return [(xa, ya)]
    if dx >= dy:
        if xa > xb:
            xa, ya, xb, yb = xb, yb, xa, ya
        return [(x, ya + (2 * (x - xa) * (yb - ya) + dx) // (2 * dx)) for x in range(xa, xb + 1)]
    if ya > yb:
        xa, ya, xb, yb = xb, yb, xa, ya
    return [(xa + (2 * (y - ya) * (xb - xa) + dy) // (2 * dy), y) for y in range(ya, yb + 1)]


def nearest_walk(xa: int, ya: int, xb: int, yb: int) -> tuple[list, int]:
    """The same line by brute force: along the major axis from the smaller end, the candidate minor coordinate nearest to the exact
    rational position, an exact tie to the larger one.  -> (pixels, number of exact ties met)."""
    dx, dy = abs(xb - xa), abs(yb - ya)
    if dx == 0 and dy == 0:
        return [(xa, ya)], 0
    swap = dx < dy
    if swap:
        xa, ya, xb, yb = ya, xa, yb, xb
    if xa > xb:
        xa, ya, xb, yb = xb, yb, xa, ya
    out, ties = [], 0
    for x in range(xa, xb + 1):
        exact = ya + Fraction((x - xa) * (yb - ya), xb - xa)
        lo = exact.numerator // exact.denominator
        best = min(range(lo - 1, lo + 3), key=lambda c: (abs(c - exact), -c))
        ties += abs(best - exact) == Fraction(1, 2)
        out.append((best, x) if swap else (x, best))
    return out, ties


def line_mask(xa, ya, xb, yb, h: int, w: int) -> np.ndarray:
    m = np.zeros((h, w), bool)
    for x, y in line_pixels(xa, ya, xb, yb):
        if 0 <= x < w and 0 <= y < h:
            m[y, x] = True
    return m


def shape_mask(row, toggles, h: int, w: int) -> np.ndarray:
    kind, _, a, b, c, d = (int(v) for v in row[:6])
    if kind == FILL:
        return fill_mask(np.asarray(toggles)[a:a + b], h, w)
    return line_mask(a, b, c, d, h, w)


def blend(image: np.ndarray, overlay: np.ndarray, w0, w1) -> np.ndarray:
    """rintf(image * w0 + overlay * w1) in fp32, each operation rounded on its own, clamped to 0..255."""
    a = image.astype(np.float32) * np.float32(w0)
    b = overlay.astype(np.float32) * np.float32(w1)
    return np.clip(np.rint(a + b), 0, 255).astype(np.uint8)


def overlay(image: np.ndarray, shapes, toggles, w0, w1, bgr: bool = False) -> np.ndarray:
    """One frame by the rule: uint8 [h,w,3] RGB -> uint8 [h,w,3] (B,G,R when `bgr`)."""
    image = np.asarray(image, np.uint8)
    h, w = image.shape[:2]
    ov = image.copy()
    for row in np.asarray(shapes, np.int64).reshape(-1, 8):
        colour = int(row[1])
        ov[shape_mask(row, toggles, h, w)] = (colour & 255, colour >> 8 & 255, colour >> 16 & 255)
    out = blend(image, ov, w0, w1)
    return np.ascontiguousarray(out[..., ::-1]) if bgr else out


def covered(shapes, toggles, h: int, w: int) -> np.ndarray:
    """bool [h,w]: the union of all rows."""
    m = np.zeros((h, w), bool)
    for row in np.asarray(shapes, np.int64).reshape(-1, 8):
        m |= shape_mask(row, toggles, h, w)
    return m


# ---------------------------------------------------------------------------------------------------------------- test polygons
def star_polygon(rng, h: int, w: int) -> np.ndarray:
    """A star-shaped polygon with integer vertices [k,2] (x, y) around a centre inside the frame: sorted angles, random radii; vertices
    may leave the frame a little."""
    k = int(rng.integers(3, 13))
    cx, cy = rng.uniform(0.25 * w, 0.75 * w), rng.uniform(0.25 * h, 0.75 * h)
    ang = np.sort(rng.uniform(0, 2 * np.pi, k))
    rad = rng.uniform(0.1, 0.6, k) * min(h, w)
    return np.stack([np.rint(cx + rad * np.cos(ang)), np.rint(cy + rad * np.sin(ang))], 1).astype(np.int64)


def strictly_inside(poly: np.ndarray, h: int, w: int) -> np.ndarray:
    """bool [h,w]: the integer point (x, y) lies strictly inside the polygon (even-odd rule, exact in integers; points on an edge or a
    vertex are not inside)."""
    y, x = np.mgrid[0:h, 0:w].astype(np.int64)
    inside = np.zeros((h, w), bool)
    on_edge = np.zeros((h, w), bool)
    k = len(poly)
    for j in range(k):
        (x0, y0), (x1, y1) = poly[j], poly[(j + 1) % k]
        cross = (x1 - x0) * (y - y0) - (y1 - y0) * (x - x0)
        on_edge |= (cross == 0) & (x >= min(x0, x1)) & (x <= max(x0, x1)) & (y >= min(y0, y1)) & (y <= max(y0, y1))
        if y0 == y1:
            continue
        if y0 > y1:
            x0, y0, x1, y1, cross = x1, y1, x0, y0, -cross
        # the ray to +x from (x, y) crosses the upward edge iff y0 <= y < y1 and the point is left of it (cross > 0)
        inside ^= (y >= y0) & (y < y1) & (cross > 0)
    return inside & ~on_edge
