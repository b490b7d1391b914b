"""The reference of the pose overlay (hh_render_poses_u8_batch, keypoints/visualization.py): the drawing rule of include/hhrnet.h in
numpy, written from that text and not from the C++, whole frame at a time and without any bounding box; and the stand-ins that
tools/make_render_golden.py binds to cv2.ellipse / cv2.circle / cv2.addWeighted so that the reference's own plot_connections runs:
each logs its call and rasterises it by the stated rule.

cv2 is not installed where the fixtures are made: parity of the covered pixel set with cv2's rasteriser is UNPINNED (include/hhrnet.h
says how the rule deviates).  Shared by tests/test_render_cpu.py, tests/test_gpu_render.py, tools/make_render_golden.py and
tools/render_time.py."""
import math

import numpy as np

F = np.float32
DISC, RING, ELLIPSE = 0, 1, 2

COCO_LIMBS = [(15, 13), (13, 11), (16, 14), (14, 12), (11, 12), (5, 11), (6, 12), (5, 6), (5, 7), (6, 8), (7, 9), (8, 10),
              (1, 2), (0, 1), (0, 2), (1, 3), (2, 4), (3, 5), (4, 6)]


def _grid(h, w, cx, cy):
    y, x = np.mgrid[0:h, 0:w]
    return (x - cx).astype(np.int64), (y - cy).astype(np.int64)


def disc_mask(h, w, cx, cy, r):
    dx, dy = _grid(h, w, cx, cy)
    return dx * dx + dy * dy <= r * r + r


def ring_mask(h, w, cx, cy, R):
    dx, dy = _grid(h, w, cx, cy)
    d2 = dx * dx + dy * dy
    return (d2 > R * R - R) & (d2 <= R * R + R)


def ellipse_terms(h, w, cx, cy, a, b, c, s, dtype=F):
    """(lhs, rhs) of the ellipse inequality over the frame in `dtype`, in the stated operation order; c, s already rounded to fp32."""
    dx, dy = _grid(h, w, cx, cy)
    t = dtype
    fx, fy, c, s, A, B = dx.astype(t), dy.astype(t), t(c), t(s), t(2 * a + 1), t(2 * b + 1)
    u = fx * c + fy * s
    v = fy * c - fx * s
    p = (t(2) * u) * B
    q = (t(2) * v) * A
    lhs = p * p + q * q
    ab = A * B
    return lhs, ab * ab


def ellipse_mask(h, w, cx, cy, a, b, c, s):
    lhs, rhs = ellipse_terms(h, w, cx, cy, a, b, c, s)
    return lhs <= rhs


def limb_ellipse(x1, y1, x2, y2, size):
    """draw_elipsis on integer ends -> (cx, cy, a, b, c, s) with c, s rounded once to fp32."""
    cx, cy = (x1 + x2) // 2, (y1 + y2) // 2
    dx, dy = x2 - x1, y2 - y1
    hyp = math.sqrt(float(dx * dx + dy * dy))
    dist = int(hyp)
    if abs(dx) > abs(dy):
        a, b, c, s = dist // 2, size, dx / hyp, dy / hyp
    else:
        a, b = size, dist // 2
        c, s = (dy / hyp, -dx / hyp) if hyp != 0 else (1.0, 0.0)
    return cx, cy, a, b, F(c), F(s)


def blend(image, conn, alpha):
    w0, w1 = F(1.0 - float(alpha)), F(float(alpha))
    v = np.rint(image.astype(F) * w0 + conn.astype(F) * w1)
    return np.clip(v, 0, 255).astype(np.uint8)


def primitives(coords, scores, limbs, thr, color_mode, palette, *, ring_first=False, reverse_people=False, trunc_centre=False, swap_axes=False,
               strict_thr=False, size_from_drawn=False, kpts_first=False):
    """The draw list of the rule: (kind, cx, cy, a, b, c, s, colour) in draw order.  The keyword switches plant one defect each (the
    CPU test shows that the golden cases tell every one of them from the rule)."""
    coords = np.asarray(coords, np.float64)
    P = len(coords)
    out = []
    if P == 0:
        return out
    scores = np.asarray(scores, np.float64).reshape(P, -1)
    K = coords.shape[1]
    skip = (scores <= thr) if strict_thr else (scores < thr)
    order = range(P - 1, -1, -1) if reverse_people else range(P)
    for i in order:
        ys = coords[i, :, 1]
        if size_from_drawn and (~skip[i]).any():
            ys = ys[~skip[i]]
        size = max(2, int((ys.max() - ys.min()) / 100))
        xy = [(int(x), int(y)) for x, y in coords[i]]
        limb_part, kpt_part = [], []
        for j, (k0, k1) in enumerate(limbs or []):
            if skip[i, k0] or skip[i, k1]:
                continue
            (x1, y1), (x2, y2) = xy[k0], xy[k1]
            cx, cy, a, b, c, s = limb_ellipse(x1, y1, x2, y2, size)
            if trunc_centre:
                cx, cy = int((x1 + x2) / 2), int((y1 + y2) / 2)
            if swap_axes:
                a, b = b, a
            limb_part.append((ELLIPSE, cx, cy, a, b, c, s, tuple(int(v) for v in palette[i if color_mode == "person" else j][:3])))
        for j in range(K):
            if skip[i, j]:
                continue
            x, y = xy[j]
            colour = tuple(int(v) for v in palette[i if color_mode == "person" else j][:3])
            pair = [(DISC, x, y, size, size, F(1), F(0), colour), (RING, x, y, size + 1, size + 1, F(1), F(0), (0, 0, 0))]
            kpt_part += pair[::-1] if ring_first else pair
        out += kpt_part + limb_part if kpts_first else limb_part + kpt_part
    return out


def draw(conn, prim):
    kind, cx, cy, a, b, c, s, colour = prim
    h, w = conn.shape[:2]
    m = disc_mask(h, w, cx, cy, a) if kind == DISC else ring_mask(h, w, cx, cy, a) if kind == RING else ellipse_mask(h, w, cx, cy, a, b, c, s)
    conn[m] = colour


def render(image, coords, scores, limbs, thr, color_mode, alpha, palette, **defect):
    """plot_connections by the stated rule -> uint8 [h,w,3]."""
    conn = image.copy()
    for prim in primitives(coords, scores, limbs, thr, color_mode, palette, **defect):
        draw(conn, prim)
    return blend(image, conn, alpha)


def render_prims(image, prims, alpha, bgr=False):
    """The same from an explicit draw list."""
    conn = image.copy()
    for prim in prims:
        draw(conn, prim)
    out = blend(image, conn, alpha)
    return np.ascontiguousarray(out[..., ::-1]) if bgr else out


def from_table(table):
    """An hh_render_prim table (structured array) -> draw list; the table's bounding boxes are dropped."""
    out = []
    for p in table:
        e = int(p["kind"]) == ELLIPSE
        out.append((int(p["kind"]), int(p["cx"]), int(p["cy"]), (int(p["A"]) - 1) // 2 if e else int(p["A"]), (int(p["B"]) - 1) // 2 if e else int(p["B"]),
                    F(p["c"]), F(p["s"]), tuple(int(v) for v in p["rgb"])))
    return out


# ---------------------------------------------------------------- stand-ins for cv2 (tools/make_render_golden.py)
# A logged call is one float64 row (every field is an integer or a double, so the rows are exact):
#   ellipse      (0, cx, cy, a, b, angle in degrees, r, g, b, thickness)
#   circle       (1, cx, cy, radius, radius, 0, r, g, b, thickness)        thickness -1 = filled disc, 1 = ring
#   addWeighted  (2, w0, w1, 0, 0, 0, 0, 0, 0, 0)                          the doubles the reference passed: 1 - alpha, alpha
CALL_ELLIPSE, CALL_CIRCLE, CALL_BLEND, ANGLE_COL = 0, 1, 2, 5


class Recorder:
    """cv2.ellipse / cv2.circle / cv2.addWeighted as the reference's plot_connections calls them: log + rasterise by the rule."""

    def __init__(self):
        self.calls = []

    def ellipse(self, img, center, axes, angle, start, end, color, thickness):
        assert (start, end, thickness) == (0, 360, -1)
        cx, cy, a, b = int(center[0]), int(center[1]), int(axes[0]), int(axes[1])
        assert (cx, cy, a, b) == (center[0], center[1], axes[0], axes[1])
        self.calls.append((CALL_ELLIPSE, cx, cy, a, b, float(angle)) + tuple(int(v) for v in color) + (thickness,))
        # (only the stand-in's pixels use cos / sin of the logged angle; the product's table is compared to the angle itself, and the
        # golden tool asserts that the image equals `render`, which forms c and s by the rule)
        rad = float(angle) * math.pi / 180.0
        draw(img, (ELLIPSE, cx, cy, a, b, F(math.cos(rad)), F(math.sin(rad)), tuple(int(v) for v in color)))
        return img

    def circle(self, img, center, radius, color, thickness):
        assert thickness in (-1, 1) and int(radius) == radius
        cx, cy = int(center[0]), int(center[1])
        self.calls.append((CALL_CIRCLE, cx, cy, int(radius), int(radius), 0.0) + tuple(int(v) for v in color) + (thickness,))
        draw(img, (DISC if thickness == -1 else RING, cx, cy, int(radius), int(radius), F(1), F(0), tuple(int(v) for v in color)))
        return img

    def addWeighted(self, src1, alpha, src2, beta, gamma):
        assert gamma == 0
        self.calls.append((CALL_BLEND, float(alpha), float(beta), 0, 0, 0.0, 0, 0, 0, 0))
        v = np.rint(src1.astype(F) * F(alpha) + src2.astype(F) * F(beta))
        return np.clip(v, 0, 255).astype(np.uint8)

    def rows(self):
        return np.array(self.calls, np.float64).reshape(-1, 10)


def calls_of_table(table, directions, alpha):
    """What the recorder would have logged for a product table (build_primitives(..., return_direction=True)); the angle column is
    atan2(s, c) in degrees of the float64 direction."""
    rows = []
    for p, (c, s) in zip(table, directions):
        kind = int(p["kind"])
        colour = tuple(int(v) for v in p["rgb"])
        if kind == ELLIPSE:
            rows.append((CALL_ELLIPSE, int(p["cx"]), int(p["cy"]), (int(p["A"]) - 1) // 2, (int(p["B"]) - 1) // 2, math.degrees(math.atan2(s, c))) + colour + (-1,))
        else:
            rows.append((CALL_CIRCLE, int(p["cx"]), int(p["cy"]), int(p["A"]), int(p["B"]), 0.0) + colour + (-1 if kind == DISC else 1,))
    rows.append((CALL_BLEND, 1 - float(alpha), float(alpha), 0, 0, 0.0, 0, 0, 0, 0))
    return np.array(rows, np.float64).reshape(-1, 10)


def calls_of_prims(prims, alpha):
    """The same for a draw list of `primitives` (the rule's own, or one with a planted defect).  Every column but the angle is exact;
    the angle is atan2 of the fp32 direction, good to 2^-24 rad = 3.4e-6 degrees."""
    rows = []
    for kind, cx, cy, a, b, c, s, colour in prims:
        if kind == ELLIPSE:
            rows.append((CALL_ELLIPSE, cx, cy, a, b, math.degrees(math.atan2(float(s), float(c)))) + tuple(colour) + (-1,))
        else:
            rows.append((CALL_CIRCLE, cx, cy, a, b, 0.0) + tuple(colour) + (-1 if kind == DISC else 1,))
    rows.append((CALL_BLEND, 1 - float(alpha), float(alpha), 0, 0, 0.0, 0, 0, 0, 0))
    return np.array(rows, np.float64).reshape(-1, 10)


def same_calls(mine, recorded, angle_tol=1e-5):
    """Two call lists agree: same length, every field but the angle exact, the angle (modulo 360) within `angle_tol` degrees."""
    if mine.shape != recorded.shape:
        return False
    other = [k for k in range(10) if k != ANGLE_COL]
    diff = np.abs((mine[:, ANGLE_COL] - recorded[:, ANGLE_COL] + 180.0) % 360.0 - 180.0)
    return bool(np.array_equal(mine[:, other], recorded[:, other]) and (diff <= angle_tol).all())
