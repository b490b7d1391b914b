"""A numpy restatement of the rule written at hh_pose_score_batch in include/hhrnet.h (per-image OKS / PCKh against annotations), written
from the header and from nothing else: not the code under test.  Every fp64 operation is one numpy operation (so it rounds on its own),
every sum is a Python loop in the stated order.  `defect` plants one named deviation (DEFECTS) so that the tests can show that the
lattice notices it."""
import numpy as np

NONFINITE, NO_PRED = 1, 2
FALLBACK = 1
SPACING = 2.0 ** -52

DEFECTS = ("descending_walk", "ge", "no_mask", "area_no_spacing", "vars_no_2", "no_round", "f32_skipped", "f32_on_fallback")


def polygon_area(poly) -> float:
    """|sum x_prev*y - y_prev*x| * 0.5 over the coordinates truncated toward zero, in exact integers; 0 below three points."""
    pts = [(int(np.trunc(x)), int(np.trunc(y))) for x, y in np.asarray(poly, np.float64).reshape(-1, 2)]
    if len(pts) < 3:
        return 0.0
    total = 0
    for j, (x, y) in enumerate(pts):
        xp, yp = pts[j - 1]
        total += xp * y - yp * x
    return float(abs(total)) * 0.5


def object_area(polygons, defect=None) -> float:
    area = 0.0
    for poly in polygons or []:
        area = area + polygon_area(poly)
    return area if defect == "area_no_spacing" else area + SPACING


def unwarp(xy, M, fallback: bool, defect=None) -> np.ndarray:
    """DECODE form: float32 [P,K,2] model-input coordinates -> float64 [P,K,2] as the rule reads them."""
    xy = np.asarray(xy, np.float32)
    x, y = xy[..., 0].astype(np.float64), xy[..., 1].astype(np.float64)
    M = np.asarray(M, np.float64)
    one = np.float64(1.0)
    ux = M[0] * x + M[1] * y + M[2] * one
    uy = M[3] * x + M[4] * y + M[5] * one
    out = np.stack([ux, uy], -1)
    to_f32 = not fallback
    if defect == "f32_skipped":
        to_f32 = False
    if defect == "f32_on_fallback":
        to_f32 = True
    return out.astype(np.float32).astype(np.float64) if to_f32 else out


def decode_preds(joints, scores, num, flags, M, b: int, defect=None):
    """Image b of hh_decode's outputs -> (xy float64 [P,K,2], score float64 [P])."""
    P = max(0, min(int(num[b]), joints.shape[1]))
    fb = bool(flags is not None and int(flags[b]) & FALLBACK)
    xy = unwarp(joints[b, :P, :, :2], M[b], fb, defect)
    if fb:
        K = joints.shape[2]
        s = np.float64(0.0)
        for _ in range(K):
            s = s + np.float64(0.01)
        sc = np.full(P, s / np.float64(K))
    else:
        sc = scores[b, :P].astype(np.float64)
    return xy, sc


def walk_order(score, defect=None) -> list:
    order = sorted(range(len(score)), key=lambda p: (score[p], p))  # ascending, stable
    return order[::-1] if defect == "descending_walk" else order


def score_image(pxy, pscore, t_xyv, t_area, t_head, variances, alpha=0.5, metric="oks", defect=None) -> dict:
    """One image: pxy float64 [P,K,2], pscore float64 [P], targets [T,K,3], [T], [T] -> dict(value, obj [T], kpt [T,K], match [T], status)."""
    pxy, pscore, t_xyv = np.asarray(pxy, np.float64), np.asarray(pscore, np.float64), np.asarray(t_xyv, np.float64)
    P, T, K = len(pscore), len(t_xyv), t_xyv.shape[1] if t_xyv.ndim == 3 else pxy.shape[1]
    status = (NONFINITE if not (np.isfinite(pxy).all() and np.isfinite(pscore).all()) else 0) | (NO_PRED if P == 0 and T > 0 else 0)
    if status:
        return {"value": np.nan, "obj": np.full(T, np.nan), "kpt": np.full((T, K), np.nan), "match": np.full(T, -1, np.int32), "status": status}
    obj, kpt, match = np.zeros(T), np.zeros((T, K)), np.zeros(T, np.int32)
    order = walk_order(pscore, defect)
    for t in range(T):
        vis = t_xyv[t, :, 2] > 0
        mask = np.ones(K, bool) if defect == "no_mask" else vis
        n = np.float64(int(mask.sum()))
        best, m = -np.inf, -1
        for p in order:
            total = np.float64(0.0)
            for k in range(K):
                if mask[k]:
                    dx, dy = pxy[p, k, 0] - t_xyv[t, k, 0], pxy[p, k, 1] - t_xyv[t, k, 1]
                    total = total + (dx * dx + dy * dy)
            with np.errstate(divide="ignore"):
                val = np.float64(1.0) / (total / n)
            if (val >= best) if defect == "ge" else (val > best):
                best, m = val, p
        match[t] = m
        if metric == "pckh" and t_head[t] == 0:
            obj[t], kpt[t] = -1.0, -1.0
            continue
        total = np.float64(0.0)
        for k in range(K):
            if not mask[k]:
                kpt[t, k] = -1.0
                continue
            px, py, tx, ty = pxy[m, k, 0], pxy[m, k, 1], t_xyv[t, k, 0], t_xyv[t, k, 1]
            if metric == "oks":
                dx, dy = px - tx, py - ty
                two = np.float64(1.0 if defect == "vars_no_2" else 2.0)
                with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
                    e = (dx * dx + dy * dy) / ((two * np.float64(variances[k])) * np.float64(t_area[t]))
                term = np.exp(-e)
            else:
                h = np.float64(t_head[t])
                dx, dy = px / h - tx / h, py / h - ty / h
                term = np.float64(1.0 if np.sqrt(dx * dx + dy * dy) < alpha else 0.0)
            kpt[t, k] = term
            total = total + term
        obj[t] = total / n
    total, cnt = np.float64(0.0), 0
    for t in range(T):
        if metric == "oks":
            total, cnt = total + (obj[t] if defect == "no_round" else np.rint(obj[t] * 1000.0) / 1000.0), cnt + 1
        elif obj[t] != -1:
            total, cnt = total + obj[t], cnt + 1
    return {"value": float(total / cnt) if cnt else -1.0, "obj": obj, "kpt": kpt, "match": match, "status": 0}
