"""Shared by tests/test_pose_score_cpu.py and tests/test_gpu_pose_score.py: a seeded lattice of small batches for hh_pose_score_batch,
the restatement's results on them (tests/pose_score_ref.py, computed once per case), a DERIVED budget for every object OKS, and the
separation conditions under which match indices, the rounded OKS and PCKh can fairly be demanded to be EXACT.

The budget (oks_budget).  For target t and its matched prediction both sides (the reference's object_OKS in numpy, the restatement, and
csrc/pose_score_math.h on the host or the device) form e_k = d2_k / ((2 vars_k) area_t) in fp64 with every operation rounded on its own
and in the same order, so e_k is bit-identical BY CONSTRUCTION.  They differ in exp(-e_k) (numpy's float64 exp at up to ULP_EXP_HOST = 4
ulp, OCML's / glibc's at ULP_EXP_TEST = 1 ulp: the documented bounds tests/coco_eval_budget.py cites, imported from there), in the order
of the sum of the n <= 64 terms in [0, 1] (each side within gamma_(n-1) S of the exact sum of its own terms, Higham 4.2) and in the final
division (one rounding each):
    |oks_a - oks_b| <= [ sum_k (ULP_EXP_HOST + ULP_EXP_TEST) ulp(x_k) + 2 gamma_(n-1) S ] / n + 2 u S / n,   S = sum_k x_k (1 + 2^-40).
Nothing in it comes from running the code under test.  The image value is the mean of the ROUNDED r_t: equal r_t summed in two orders
differ by at most value_budget = 2 gamma_(T-1) sum(r) / T + 2 u sum(r) / T.

Separation (separation_violations), checked on the CPU for every lattice case; `case()` perturbs the seed until it holds and fails if it
cannot, no case is left out:
  * matching: D[p,t] is a sum of n non-negative terms divided by n; two sides that sum in different orders are each within
    d_bound = (gamma_(n-1) + u) D of the exact value.  For every target the best D and every other D either come from bit-identical
    prediction rows (then every side gives them equal values and the walk order decides) or differ by more than 2 d_bound(best) +
    2 d_bound(other).
  * rounding: no oks_t * 1000 lies within 1000 * budget + u * 1000 * oks_t of a half-integer.
  * PCKh: d_k is bit-identical up to the square root (numpy's `** 0.5` is held to 1 ulp, sqrt is exact): no d_k lies within
    2 ulp(d_k) of alpha.
"""
import functools
import importlib

import numpy as np

import pose_score_ref as ref
from coco_eval_budget import U, ULP_EXP_HOST, ULP_EXP_TEST
from conftest import PKG

IDENTITY = np.array([1.0, 0.0, 0.0, 0.0, 1.0, 0.0])
SCALED = np.array([1.7, 0.0, -3.25, 0.0, 1.7, 5.5])  # a resize-align inverse: one scale, two offsets
K3_VARS = np.array([0.004, 0.01, 0.02])
W = 4  # floats per joint row of the decode (x, y, score, one tag)


def ps():
    return importlib.import_module(PKG + ".keypoints.pose_score")


# ------------------------------------------------------------------------------------------------ pieces
def person(rs, c, K, n_vis=None):
    """An annotated person around centre c: integer coordinates (COCO stores integers), v in 0..2 with exactly n_vis labelled joints
    (random if None), an unlabelled joint stored as 0, 0, 0."""
    xy = np.round(c + rs.uniform(-40, 40, (K, 2)))
    if n_vis is None:
        v = rs.randint(0, 3, K).astype(np.float64)
        if not (v > 0).any():
            v[rs.randint(K)] = 2.0
    else:
        v = np.zeros(K)
        v[rs.permutation(K)[:n_vis]] = rs.randint(1, 3, n_vis)
    xy[v == 0] = 0.0
    return np.concatenate([xy, v[:, None]], 1)


def box_polygon(rs, c):
    w, h = rs.uniform(60, 110), rs.uniform(90, 140)
    x0, y0 = c[0] - w / 2, c[1] - h / 2
    return [[x0, y0, x0 + w, y0 + 0.4, x0 + w + 0.7, y0 + h, x0, y0 + h]]  # fractions: the area truncates them toward zero


def to_input(xy_raw, M):
    """Raw-image coordinates -> float32 model-input coordinates of a scale-and-offset inverse matrix M."""
    out = np.empty_like(xy_raw, dtype=np.float64)
    out[..., 0] = (xy_raw[..., 0] - M[2]) / M[0]
    out[..., 1] = (xy_raw[..., 1] - M[5]) / M[4]
    return out.astype(np.float32)


def image(rs, K, P, targets, M, near, noise, fallback=False, scores=None, polygons=None, heads=None):
    """One image: `targets` [T,K,3]; prediction p is a copy of target near[p] (-1: a random pose) with `noise[p]` pixels of jitter
    (0 = exactly on it under the identity matrix), moved into model-input coordinates."""
    T = len(targets)
    xy = np.zeros((P, K, 2))
    for p in range(P):
        if near[p] >= 0:
            base = targets[near[p]][:, :2].copy()
            base[targets[near[p]][:, 2] == 0] = 300.0 + 10 * p
            xy[p] = base + (rs.normal(0, noise[p], (K, 2)) if noise[p] else 0.0)
        else:
            xy[p] = 300.0 + rs.uniform(-250, 250, (K, 2))
    joints = np.zeros((P, K, W), np.float32)
    joints[..., :2] = to_input(xy, M)
    joints[..., 2:] = rs.uniform(0.1, 0.9, (P, K, W - 2))
    sc = rs.uniform(0.1, 0.9, P) if scores is None else np.asarray(scores)
    return {"joints": joints, "scores": sc.astype(np.float32), "flag": 1 if fallback else 0, "M": np.asarray(M, np.float64),
            "t_xyv": np.asarray(targets, np.float64).reshape(T, K, 3), "polygons": polygons if polygons is not None else [[] for _ in range(T)],
            "heads": heads if heads is not None else [(0, 0, 0, 0)] * T}


def people(rs, K, n_vis_list, spread=220.0):
    cs = [300.0 + rs.uniform(-spread, spread, 2) for _ in n_vis_list]
    return cs, [person(rs, c, K, n) for c, n in zip(cs, n_vis_list)]


def _generate(name, seed):
    rs = np.random.RandomState(seed)
    metric, K, variances, alpha = "oks", 17, None, 0.5
    if name == "k17_mixed":  # B = 5 with mixed P and T
        imgs = []
        # T = 1, all 17 joints, NO polygon (area 2^-52): predictions 0 and 2 sit exactly on it, 2 comes first in the walk and wins
        cs, tg = people(rs, K, [17])
        imgs.append(image(rs, K, 3, tg, IDENTITY, near=[0, 0, 0], noise=[0, 4.0, 0], scores=[0.7, 0.9, 0.4]))
        # P = M = 30, T = 7, scaled matrix; n_t = 1, 7, 8, 17; targets 5 and 6 are neighbours and only 5 has a prediction of its own
        cs, tg = people(rs, K, [1, 7, 8, 17, None, 17])
        twin = tg[5].copy()
        twin[:, :2] += 3.0
        tg.append(twin)
        near = [0, 1, 2, 3, 4, 5] + [-1] * 24
        imgs.append(image(rs, K, 30, tg, SCALED, near=near, noise=[3.0] * 30, polygons=[box_polygon(rs, c) for c in cs] + [box_polygon(rs, cs[5])]))
        # P = 2 with equal scores, T = 8, identity
        cs, tg = people(rs, K, [None] * 8)
        imgs.append(image(rs, K, 2, tg, IDENTITY, near=[0, 3], noise=[2.0, 5.0], scores=[0.5, 0.5], polygons=[box_polygon(rs, c) for c in cs]))
        # P = 1 with the fallback bit, T = 9, scaled matrix: the un-warped coordinates stay float64
        cs, tg = people(rs, K, [None] * 9, spread=60.0)
        imgs.append(image(rs, K, 1, tg, SCALED, near=[4], noise=[6.0], fallback=True, polygons=[box_polygon(rs, c) for c in cs]))
        # T = 0: the value is -1
        imgs.append(image(rs, K, 5, np.zeros((0, K, 3)), SCALED, near=[-1] * 5, noise=[0] * 5))
    elif name == "k3":  # B = 1, three joints, two exact hits with EQUAL scores: the lower index comes first in the walk
        K, variances = 3, K3_VARS
        cs, tg = people(rs, K, [3, 2])
        imgs = [image(rs, K, 3, tg, IDENTITY, near=[0, 0, 1], noise=[0, 0, 2.0], scores=[0.6, 0.6, 0.2], polygons=[box_polygon(rs, c) for c in cs])]
    elif name == "t128":  # B = 1, the most targets an image may have
        cs, tg = people(rs, K, [None] * 128, spread=2000.0)
        imgs = [image(rs, K, 30, tg, SCALED, near=list(range(0, 120, 4)), noise=[3.0] * 30, polygons=[box_polygon(rs, c) for c in cs])]
    elif name == "pckh":  # B = 2, head boxes, one of size 0
        metric = "pckh"
        cs, tg = people(rs, K, [17, 8, 1])
        cs2, tg2 = people(rs, K, [None, None])
        imgs = [image(rs, K, 4, tg, IDENTITY, near=[0, 1, 2, 0], noise=[10.0, 18.0, 3.0, 0], heads=[(10, 10, 28, 34), (5, 5, 5, 5), (0, 0, 20, 21)]),
                image(rs, K, 2, tg2, SCALED, near=[1, 0], noise=[12.0, 25.0], heads=[(0, 0, 18, 24), (3, 4, 30, 40)])]
    else:
        raise KeyError(name)
    return {"name": name, "seed": seed, "K": K, "metric": metric, "alpha": alpha, "images": imgs, "variances": ps().OKS_VARIANCES if variances is None else variances}


LATTICE = ("k17_mixed", "k3", "t128", "pckh")


# ------------------------------------------------------------------------------------------------ tables in both forms
def tables(c, defect=None):
    """The arrays of a case: hh_decode-shaped outputs padded with NaN rows that must never be read, the target tables, and the F64
    predictions (the restatement's un-warp of the same rows)."""
    imgs, K = c["images"], c["K"]
    B, Mmax = len(imgs), max(len(im["scores"]) for im in imgs)
    joints, scores = np.full((B, Mmax, K, W), np.nan, np.float32), np.full((B, Mmax), np.nan, np.float32)
    num, flags, inv = np.zeros(B, np.int32), np.zeros(B, np.int32), np.zeros((B, 6))
    for b, im in enumerate(imgs):
        P = len(im["scores"])
        joints[b, :P], scores[b, :P], num[b], flags[b], inv[b] = im["joints"], im["scores"], P, im["flag"], im["M"]
    t_off = np.cumsum([0] + [len(im["t_xyv"]) for im in imgs]).astype(np.int32)
    area = [ref.object_area(p, defect) for im in imgs for p in im["polygons"]]
    head = [ps().head_size(h) if c["metric"] == "pckh" else 0.0 for im in imgs for h in im["heads"]]
    targets = {"t_off": t_off, "t_xyv": np.concatenate([im["t_xyv"] for im in imgs]), "t_area": np.asarray(area, np.float64).reshape(-1),
               "t_head": np.asarray(head, np.float64).reshape(-1), "K": K}
    preds = [ref.decode_preds(joints, scores, num, flags, inv, b, defect) for b in range(B)]
    return {"decode": (joints, scores, num, flags), "inv_affine": inv, "targets": targets, "preds": preds}


def restated(c, defect=None):
    """The restatement on every image of the case, in the layout of the entry points' outputs."""
    t = tables(c, defect)
    tg, K = t["targets"], c["K"]
    out = {"value": [], "obj": [], "kpt": [], "match": [], "status": []}
    for b, (xy, sc) in enumerate(t["preds"]):
        a, e = tg["t_off"][b], tg["t_off"][b + 1]
        r = ref.score_image(xy, sc, tg["t_xyv"][a:e], tg["t_area"][a:e], tg["t_head"][a:e], c["variances"], c["alpha"], c["metric"], defect)
        for k in ("obj", "kpt", "match"):
            out[k].append(r[k])
        out["value"].append(r["value"])
        out["status"].append(r["status"])
    return {"value": np.asarray(out["value"]), "obj": np.concatenate(out["obj"]), "kpt": np.concatenate(out["kpt"]).reshape(-1, K),
            "match": np.concatenate(out["match"]).astype(np.int32), "status": np.asarray(out["status"], np.int32)}


# ------------------------------------------------------------------------------------------------ budget and separation
def gamma(m):
    m = np.maximum(m, 0)
    return m * U / (1 - m * U)


def oks_budget(kpt, ulps_exp=ULP_EXP_HOST + ULP_EXP_TEST):
    """[T] bound on |oks_a - oks_b| from the per-joint terms kpt [T,K] (-1 = unlabelled) of either side (module docstring).  `ulps_exp`:
    the sum of the two sides' exp bounds; 2 * ULP_EXP_TEST between the device (OCML) and the host twin (glibc)."""
    lab = kpt >= 0
    x = np.where(lab, kpt, 0.0)
    n = np.maximum(lab.sum(-1), 1)
    S = x.sum(-1) * (1 + 2.0 ** -40)
    ulps = np.where(lab, np.spacing(x), 0.0).sum(-1)
    return (ulps_exp * ulps + 2 * gamma(n - 1) * S) / n + 2 * U * S / n


def value_budget(obj, t_off):
    """[B] bound on the image value's difference between two sides that hold equal rounded r_t but sum them in different orders."""
    out = np.zeros(len(t_off) - 1)
    for b in range(len(out)):
        r = np.rint(obj[t_off[b]:t_off[b + 1]] * 1000.0) / 1000.0
        T = len(r)
        if T:
            out[b] = (2 * gamma(T - 1) + 2 * U) * np.abs(r).sum() / T
    return out


def separation_violations(c, t, r):
    """The number of places where a condition of the module docstring fails on the restatement's results r of case c (tables t)."""
    bad = 0
    tg = t["targets"]
    for b, (xy, _) in enumerate(t["preds"]):
        rows = xy.reshape(len(xy), -1).view(np.uint64)
        for j in range(tg["t_off"][b], tg["t_off"][b + 1]):
            xyv = tg["t_xyv"][j]
            vis = xyv[:, 2] > 0
            n = int(vis.sum())
            D = ((xy[:, vis] - xyv[None, vis, :2]) ** 2).sum((1, 2)) / n
            bound = (gamma(n - 1) + U) * D
            m = int(r["match"][j])
            for p in range(len(xy)):
                if p != m and not np.array_equal(rows[p], rows[m]) and abs(D[p] - D[m]) <= 2 * bound[p] + 2 * bound[m]:
                    bad += 1
            if c["metric"] == "pckh" and tg["t_head"][j] != 0:
                h = tg["t_head"][j]
                d = np.sqrt(((xy[m, vis] / h - xyv[vis, :2] / h) ** 2).sum(-1))
                bad += int((np.abs(d - c["alpha"]) <= 2 * np.spacing(d)).sum())
    if c["metric"] == "oks":
        scaled = r["obj"] * 1000.0
        bad += int((np.abs(scaled - (np.floor(scaled) + 0.5)) <= 1000.0 * oks_budget(r["kpt"]) + U * scaled).sum())
    return bad


@functools.lru_cache(maxsize=None)
def case(name):
    """(case, tables, restatement's results) with the separation conditions satisfied; the seed is perturbed until they are."""
    base = 1 + LATTICE.index(name)
    for attempt in range(20):
        c = _generate(name, base + 1000 * attempt)
        t = tables(c)
        r = restated(c)
        if separation_violations(c, t, r) == 0:
            return c, t, r
    raise AssertionError(f"{name}: no seed satisfies the separation conditions")


def over_the_maxima(what):
    """Tables that must be refused: T = 129 targets in one image, or P = 65 predictions (F64 form)."""
    rs = np.random.RandomState(7)
    K = 17
    T, P = (129, 2) if what == "targets" else (2, 65)
    _, tg = people(rs, K, [None] * T)
    targets = ps().make_targets(np.asarray(tg))
    return targets, [(rs.uniform(0, 500, (P, K, 2)), rs.uniform(0.1, 0.9, P))]
