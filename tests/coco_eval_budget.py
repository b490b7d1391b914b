"""Shared by tests/test_coco_eval_budget_cpu.py and tests/test_gpu_coco_eval.py: a seeded lattice of small synthetic COCO keypoint
datasets, the host evaluator's results on them (computed once per case), a DERIVED error budget for every OKS value, the separation
condition that makes "exactly equal match tables" a fair demand on an OKS that may differ in its last bits, adversarial OKS matrices
for the matching walk, and numpy models of planted defects.

The OKS budget (oks_budget).  For one (detection, ground truth) pair the host evaluator (`COCOKeypointsEval._oks`) and the code under
test (csrc/coco_eval_math.h, on the host or on the device) both form, per joint k that counts,
    e_k = (dx^2 + dy^2) / vars_k / (area + 2^-52) / 2
in fp64 with every operation rounded on its own and in the same order (the library is built with -ffp-contract=off), so e_k is
bit-identical BY CONSTRUCTION and contributes nothing.  They then differ in three places only:
  * x_k = exp(-e_k).  Each library's result is within its documented bound of the true value, so the two differ by at most the sum of
    the bounds, in units of ulp(x_k):
      - numpy's float64 exp is, depending on the build and the CPU, glibc's (glibc manual, "Known Maximum Errors in Math Functions":
        exp, x86_64: 1 ulp), numpy's own AVX512F kernel (its source states a maximum error of 0.52 ulp) or an SVML routine (numpy holds
        its SVML-backed float64 functions to 4 ulp).  The largest, ULP_EXP_HOST = 4, is taken.
      - the device's exp is OCML's (ROCm documentation, "HIP math API", double precision: exp, 1 ulp); compiled for the host the same
        header calls glibc's (1 ulp).  ULP_EXP_TEST = 1.
  * the sum of the n <= 64 terms, all in [0, 1], taken in two different orders (numpy adds pairwise, the header in ascending k): each
    side is within gamma_(n-1) * sum(x) of the exact sum of ITS terms, gamma_m = m u / (1 - m u), u = 2^-53 (Higham, Accuracy and
    Stability of Numerical Algorithms, section 4.2).
  * the final division by n: one rounding on each side, u * |result| each.
So  |oks_host - oks_test| <= [ sum_k (ULP_EXP_HOST + ULP_EXP_TEST) ulp(x_k) + 2 gamma_(n-1) S ] / n + 2 u S / n,  S = sum_k x_k (1 + 2^-40)
(the factor covers S being evaluated from the host's own rounded terms).  It is evaluated per pair from the pair's operands; nothing in
it comes from running the code under test.

The separation condition (separation_violations).  Match tables can only be required to be EQUAL where no decision of the walk hangs
on the last bits of an OKS value: every host value lies further than twice its budget from every start value min(t, 1 - 1e-10), and
any two values of one detection's row either come from bit-identical operands (then both sides give them equal values) or lie further
apart than the sum of their budgets.  `case()` perturbs the seed until the host reference satisfies it and fails if it cannot; no case
is dropped.  The walk itself must not depend on it: adversarial_oks() violates it on purpose and is fed to the matching alone.
"""
import functools
import importlib

import numpy as np

from conftest import PKG

ULP_EXP_HOST, ULP_EXP_TEST = 4.0, 1.0
U = 2.0 ** -53
K1_SIGMAS = np.array([0.05])


def ce():
    return importlib.import_module(PKG + ".keypoints.coco_eval")


# ------------------------------------------------------------------------------------------------ dataset pieces
def gt_person(img, ann_id, xyv, area, iscrowd=0, bbox=None):
    xyv = np.asarray(xyv, np.float64)
    vis = xyv[:, 2] > 0
    if bbox is None:
        p = xyv[vis] if vis.any() else xyv
        bbox = [float(p[:, 0].min()), float(p[:, 1].min()), float(np.ptp(p[:, 0])), float(np.ptp(p[:, 1]))]
    return {"image_id": img, "id": ann_id, "category_id": 1, "iscrowd": iscrowd, "area": float(area), "num_keypoints": int(vis.sum()),
            "keypoints": xyv.reshape(-1).tolist(), "bbox": [float(b) for b in bbox]}


def det(img, xy, score):
    xy = np.asarray(xy, np.float64)
    return {"image_id": img, "category_id": 1, "score": float(score), "keypoints": np.concatenate([xy, np.ones((len(xy), 1))], 1).reshape(-1).tolist()}


class _Builder:
    """Images of one case.  Geometry: all people of an image sit within +-0.6 s of a centre near 1e3, s = sqrt(the image's smallest
    ground-truth area), so that no exponent e passes ~600 and no OKS underflows to an exact 0 shared by two ground truths."""

    def __init__(self, seed, K):
        self.rs, self.K, self.gts, self.dets, self.next_id, self.img = np.random.RandomState(seed), K, [], [], 1000, 0

    def pose(self, c, s, vis=True):
        xy = c + s * self.rs.uniform(-0.6, 0.6, (self.K, 2))
        v = self.rs.randint(0, 3, self.K).astype(np.float64) if vis else np.full(self.K, 2.0)
        if not (v > 0).any():
            v[self.rs.randint(self.K)] = 1.0
        xy[v == 0] = 0.0  # COCO stores an unlabelled joint as 0, 0, 0
        return np.concatenate([xy, v[:, None]], 1)

    def add_gt(self, xyv, area, **kw):
        self.next_id += 1
        self.gts.append(gt_person(self.img, self.next_id, xyv, area, **kw))

    def image(self, D, G, areas=(150.0 ** 2,), score_step=None):
        """A generic image: G ground truths with areas cycling through `areas`, D detections, detection d a jittered copy of
        ground truth d % G (jitter 0 = an OKS of exactly 1).  score_step rounds the scores, which makes equal scores."""
        self.img += 1
        rs = self.rs
        c = 1000.0 + rs.uniform(-50, 50, 2)
        s = np.sqrt(min(areas))
        poses = []
        for g in range(G):
            p = self.pose(c, s)
            poses.append(p)
            self.add_gt(p, areas[g % len(areas)], iscrowd=int(rs.rand() < 0.08))
        for d in range(D):
            if G:
                base = poses[d % G][:, :2].copy()
                base[poses[d % G][:, 2] == 0] = c
                xy = base + s * rs.choice([0.0, 0.01, 0.05, 0.2]) * rs.normal(0, 1, (self.K, 2))
            else:
                xy = c + s * rs.uniform(-0.6, 0.6, (self.K, 2))
            sc = rs.uniform(0.05, 1.0)
            self.dets.append(det(self.img, xy, np.round(sc / score_step) * score_step if score_step else sc))
        return self.img


def _special_images(b: _Builder):
    """The hand-placed situations (K = 17)."""
    rs, K = b.rs, b.K
    # crowd: several detections match one crowd ground truth; a normal one next to it
    b.img += 1
    c = np.array([1000.0, 980.0])
    crowd, normal = b.pose(c, 100.0, vis=False), b.pose(c + 30, 100.0, vis=False)
    b.add_gt(crowd, 150.0 ** 2, iscrowd=1)
    b.add_gt(normal, 150.0 ** 2)
    for d in range(4):
        b.dets.append(det(b.img, crowd[:, :2] + rs.normal(0, 2.0 + d, (K, 2)), 0.9 - 0.1 * d))
    b.dets.append(det(b.img, normal[:, :2] + rs.normal(0, 2.0, (K, 2)), 0.45))
    # break rule: the ignored (crowd) ground truth comes FIRST in annotation order and fits the detection perfectly; the real one fits
    # at about 0.83 (every joint moved in x by sqrt(-2 ln 0.83) * 2 sigma_k * sqrt(area), i.e. e_k = -ln 0.83).  The partition walks the
    # real one first, and the break keeps the match there at every threshold it passes although the ignored one scores higher.
    b.img += 1
    first = b.pose(c, 100.0, vis=False)
    second = first.copy()
    second[:, 0] += 60.0 * np.sqrt(-2 * np.log(0.83)) * 2 * ce().KPT_OKS_SIGMAS
    b.add_gt(first, 60.0 ** 2, iscrowd=1)
    b.add_gt(second, 60.0 ** 2)
    b.dets.append(det(b.img, first[:, :2], 0.8))
    b.dets.append(det(b.img, first[:, :2] + 0.5, 0.7))
    # tie: two bit-identical ground truths; the later one must take the first detection, the earlier one the second
    b.img += 1
    twin = b.pose(c, 100.0)
    b.add_gt(twin, 150.0 ** 2)
    b.add_gt(b.pose(c + 5, 100.0), 150.0 ** 2)
    b.add_gt(twin, 150.0 ** 2)
    for d in range(3):
        xy = twin[:, :2].copy()
        xy[twin[:, 2] == 0] = c
        b.dets.append(det(b.img, xy + rs.normal(0, 3.0, (K, 2)), 0.6))  # equal scores as well: the stable order decides
    # no labelled joint: the doubled-box branch, with detections inside, on the edge of and outside the doubled box
    b.img += 1
    bx, by, bw, bh = 900.0, 950.0, 64.0, 32.0
    b.add_gt(np.zeros((K, 3)), 150.0 ** 2, bbox=[bx, by, bw, bh])
    b.add_gt(b.pose(np.array([bx + 20, by + 10]), 100.0), 150.0 ** 2)
    inside = np.stack([rs.uniform(bx - bw, bx + 2 * bw, K), rs.uniform(by - bh, by + 2 * bh, K)], 1)
    edge = inside.copy()
    edge[0::2, 0], edge[1::2, 0], edge[0::3, 1], edge[1::3, 1] = bx - bw, bx + 2 * bw, by - bh, by + 2 * bh
    outside = inside.copy()
    outside[0::2, 0], outside[1::2, 1] = bx - bw - 7.0, by + 2 * bh + 11.0
    between = inside.copy()  # outside the single box, inside the doubled one
    between[:, 0], between[:, 1] = bx + bw + 0.5 * bw, by - 0.5 * bh
    for d, xy in enumerate((inside, edge, outside, between)):
        b.dets.append(det(b.img, xy, 0.9 - 0.1 * d))
    # areas exactly 32^2 and 96^2 and one ulp on either side, ground truths and detections.  A detection's area is the product of its
    # extents: joints at (0, 0) and (1, h) make it exactly h; these detections stay unmatched, so their flag is the area test itself.
    edges = [np.nextafter(v, w) for v in (32.0 ** 2, 96.0 ** 2) for w in (0.0, v, np.inf)]
    for h in edges:
        b.img += 1
        p = b.pose(c, 30.0, vis=False)
        b.add_gt(p, h)
        b.dets.append(det(b.img, p[:, :2] + rs.normal(0, 0.5, (K, 2)), 0.55))
        xy = np.stack([rs.uniform(0.1, 0.9, K), rs.uniform(0.1, 0.9, K) * h], 1)
        xy[0], xy[1] = (0.0, 0.0), (1.0, h)
        b.dets.append(det(b.img, xy, 0.5))


def _generate(name, seed):
    if name == "k17_small":  # every D x G of the small counts: images with ground truths and no detections and the reverse
        b = _Builder(seed, 17)
        for D in (0, 1, 3):
            for G in (0, 1, 2):
                b.image(D, G, areas=(150.0 ** 2, 40.0 ** 2), score_step=0.25)
    elif name == "k17_special":
        b = _Builder(seed, 17)
        _special_images(b)
    elif name == "k17_words":  # G across the 64-bit word of the taken-set; D = 25 is cut to 20
        b = _Builder(seed, 17)
        for D, G in ((20, 63), (25, 64), (3, 65), (20, 128), (1, 128), (25, 2)):
            b.image(D, G, areas=(150.0 ** 2, 50.0 ** 2, 20.0 ** 2), score_step=0.1 if G == 64 else None)
    elif name == "k17_areas":  # areas from 1 to 1e6: OKS from about 0 to exactly 1
        b = _Builder(seed, 17)
        for area in (1.0, 10.0, 1e3, 1e4, 1e5, 1e6):
            b.image(3, 3, areas=(area, area * 1.5))
        b.image(20, 2, areas=(1.0, 1e6))
    elif name == "k1":  # one joint: a detection's area is 0
        b = _Builder(seed, 1)
        for D, G in ((1, 1), (3, 2), (0, 3), (3, 0), (25, 65), (20, 128), (20, 63), (1, 64)):
            b.image(D, G, areas=(150.0 ** 2, 50.0 ** 2))
    else:
        raise KeyError(name)
    return {"name": name, "seed": seed, "K": b.K, "gts": b.gts, "dets": b.dets, "sigmas": ce().KPT_OKS_SIGMAS if b.K == 17 else K1_SIGMAS}


LATTICE = ("k17_small", "k17_special", "k17_words", "k17_areas", "k1")
LARGEST = "k17_words"


# ------------------------------------------------------------------------------------------------ host reference, budget, separation
def reference(c):
    """The host evaluator on a case, once: per image the OKS matrix, per area the evaluateImg dict; precision / recall / stats."""
    mod = ce()
    gt_imgs = sorted({g["image_id"] for g in c["gts"]} | {d["image_id"] for d in c["dets"]})
    ev = mod.COCOKeypointsEval(c["gts"], c["dets"], img_ids=gt_imgs, sigmas=c["sigmas"])
    oks = {i: ev._oks(i) for i in ev.img_ids}
    imgs = {a: {i: ev._evaluate_img(i, oks[i], rng, mod.MAX_DETS[-1]) for i in ev.img_ids} for a, rng in enumerate(mod.AREA_RNG)}
    stats = ev.evaluate().copy()
    return {"ev": ev, "img_ids": gt_imgs, "oks": oks, "imgs": imgs, "precision": ev.precision.copy(), "recall": ev.recall.copy(), "stats": stats}


def oks_terms(t, i, variant=None):
    """The per-joint exponents e [D,G,K] of image i of packed tables t and the mask of the joints that count, in _oks' operation order
    (elementwise numpy: the same roundings as the per-pair code).  `variant`: a planted defect, see DEFECTS."""
    d0, d1, g0, g1 = t["dt_off"][i], t["dt_off"][i + 1], t["gt_off"][i], t["gt_off"][i + 1]
    xd, yd = t["dt_xy"][d0:d1, None, :, 0], t["dt_xy"][d0:d1, None, :, 1]
    g = t["gt_xyv"][g0:g1][None]
    xg, yg, vg = g[..., 0], g[..., 1], g[..., 2]
    lab = (vg >= 0) if variant == "v_ge_0" else (vg > 0)
    k1 = lab.sum(-1, keepdims=True)
    bb = t["gt_bbox"][g0:g1]
    f = 1.0 if variant == "single_box" else 2.0
    x0, x1 = (bb[:, 0] - bb[:, 2] * (f - 1.0))[None, :, None], (bb[:, 0] + bb[:, 2] * f)[None, :, None]
    y0, y1 = (bb[:, 1] - bb[:, 3] * (f - 1.0))[None, :, None], (bb[:, 1] + bb[:, 3] * f)[None, :, None]
    z = 0.0
    dx = np.where(k1 > 0, xd - xg, np.maximum(z, x0 - xd) + np.maximum(z, xd - x1))
    dy = np.where(k1 > 0, yd - yg, np.maximum(z, y0 - yd) + np.maximum(z, yd - y1))
    vars_ = t["vars"] / 4.0 if variant == "sigma" else t["vars"]
    e = (dx ** 2 + dy ** 2) / vars_ / (t["gt_area"][g0:g1][None, :, None] + np.spacing(1))
    if variant != "no_half":
        e = e / 2
    counts = np.broadcast_to(np.where(k1 > 0, lab, True), e.shape)
    return e, counts


def oks_budget(t, i):
    """[D,G] bound on |host OKS - OKS under test| for image i, from the operands (module docstring)."""
    e, counts = oks_terms(t, i)
    x = np.where(counts, np.exp(-e), 0.0)
    n = counts.sum(-1)
    S = x.sum(-1) * (1 + 2.0 ** -40)
    ulps = np.where(counts, np.spacing(x), 0.0).sum(-1)
    m = np.maximum(n - 1, 0)
    gamma = m * U / (1 - m * U)
    return ((ULP_EXP_HOST + ULP_EXP_TEST) * ulps + 2 * gamma * S) / n + 2 * U * S / n


def oks_model(t, i, variant):
    """[D,G] OKS of image i from a numpy model that is NOT the code under test: "nudged" = fp64, the sum taken in descending k and
    every exp pushed to its combined bound (must stay inside the budget); the others are the planted defects (must leave it)."""
    if variant == "fp32":
        t = dict(t, **{k: t[k].astype(np.float32) for k in ("dt_xy", "gt_xyv", "gt_bbox", "gt_area", "vars")})
    e, counts = oks_terms(t, i, variant)
    x = np.exp(-e)
    if variant == "fp32":
        x = x.astype(np.float32)
    if variant == "nudged":
        sign = np.where(np.arange(x.shape[-1]) % 2 == 0, 1.0, -1.0)
        x = x + sign * (ULP_EXP_HOST + ULP_EXP_TEST) * np.spacing(x)
    x = np.where(counts, x, 0)
    n = x.shape[-1] if variant == "mean_over_K" else counts.sum(-1)
    total = np.zeros(x.shape[:-1], x.dtype)
    for k in range(x.shape[-1] - 1, -1, -1):
        total = total + x[..., k]
    return (total / n).astype(np.float64)


# planted defect -> (case, why it shows there)
DEFECTS = {
    "fp32": "k17_areas",          # coordinates near 1e3 in fp32 carry 6e-5 of error: e moves by far more than 1e-15
    "sigma": "k17_small",         # sigma instead of 2 sigma: e four times larger
    "no_half": "k17_small",       # e twice larger
    "v_ge_0": "k17_small",        # unlabelled joints (stored at 0, 0: far from any detection) enter the mean as ~0 terms
    "mean_over_K": "k17_small",   # the sum over the labelled joints divided by 17
    "single_box": "k17_special",  # the detection between the single and the doubled box is no longer at distance 0
}


def host_oks_flat(t, ref):
    """The host evaluator's OKS in the concatenated layout of hh_coco_oks."""
    out = np.zeros(int(t["oks_off"][-1]))
    for i, img in enumerate(t["img_ids"]):
        o = np.asarray(ref["oks"][int(img)], np.float64)
        out[t["oks_off"][i]:t["oks_off"][i + 1]] = o.reshape(-1)
    return out


def budget_flat(t):
    return np.concatenate([oks_budget(t, i).reshape(-1) for i in range(len(t["img_ids"]))] + [np.zeros(0)])


def separation_violations(t, ref):
    """The number of places where the separation condition of the module docstring fails on the host reference."""
    bad = 0
    starts = np.minimum(np.asarray(t["thr"]), 1 - 1e-10)
    for i, img in enumerate(t["img_ids"]):
        o = np.asarray(ref["oks"][int(img)], np.float64)
        if o.size == 0:
            continue
        bud = oks_budget(t, i)
        bad += int((np.abs(o[:, :, None] - starts[None, None, :]) <= 2 * bud[:, :, None]).sum())
        g0, g1 = t["gt_off"][i], t["gt_off"][i + 1]
        ops = np.concatenate([t["gt_xyv"][g0:g1].reshape(g1 - g0, -1), t["gt_bbox"][g0:g1], t["gt_area"][g0:g1, None]], 1).view(np.uint64)
        same = (ops[:, None, :] == ops[None, :, :]).all(-1)  # bit-identical operands (the detection is shared by the row)
        close = np.abs(o[:, :, None] - o[:, None, :]) <= bud[:, :, None] + bud[:, None, :]
        bad += int((close & ~same[None]).sum())
    return bad


@functools.lru_cache(maxsize=None)
def case(name):
    """(case, packed tables, host reference) with the separation condition satisfied; the seed is perturbed until it is."""
    mod = ce()
    base = 1 + LATTICE.index(name)
    for attempt in range(40):
        c = _generate(name, base + 1000 * attempt)
        ref = reference(c)
        t = mod.pack_tables(c["gts"], c["dets"], img_ids=ref["img_ids"], sigmas=c["sigmas"])
        if separation_violations(t, ref) == 0:
            return c, t, ref
    raise AssertionError(f"{name}: no seed satisfies the separation condition")


def refusal_case():
    """One image with 33 detections (over HH_COCO_MAX_DET): packed without the cut, only to be refused."""
    b = _Builder(99, 17)
    b.image(33, 2)
    return ce().pack_tables(b.gts, b.dets, max_det=33)


# ------------------------------------------------------------------------------------------------ expectations in table layout
def expected_tables(t, ref, oks_by_image=None):
    """dt ids matched -> ground-truth ids [A,T,N] (0 = none), dt_ignore [A,T,N], gt_ignore [A,M] in annotation order, from
    _evaluate_img.  oks_by_image: matrices to match on instead of the evaluator's own (the adversarial ones)."""
    mod = ce()
    A, T, N, M = len(mod.AREA_RNG), len(mod.IOU_THRS), len(t["dt_score"]), len(t["gt_area"])
    dtm, dti, gti = np.zeros((A, T, N), np.int64), np.zeros((A, T, N), bool), np.zeros((A, M), bool)
    ev = ref["ev"]
    for a, rng in enumerate(mod.AREA_RNG):
        for i, img in enumerate(t["img_ids"]):
            img = int(img)
            e = ref["imgs"][a][img] if oks_by_image is None else ev._evaluate_img(img, oks_by_image[img], rng, mod.MAX_DETS[-1])
            if e is None:
                continue
            d0, d1, g0, g1 = t["dt_off"][i], t["dt_off"][i + 1], t["gt_off"][i], t["gt_off"][i + 1]
            dtm[a, :, d0:d1], dti[a, :, d0:d1] = e["dtMatches"], e["dtIgnore"]
            g_ign = [1 if (g["ignore"] or g["area"] < rng[0] or g["area"] > rng[1]) else 0 for g in ev._gts[img]]
            assert np.array_equal(np.sort(g_ign, kind="mergesort"), e["gtIgnore"])
            gti[a, g0:g1] = g_ign
    return dtm, dti, gti


def match_ids(t, dt_match):
    """dt_match (row of the ground-truth table + 1) -> annotation ids, 0 = none."""
    ids = np.concatenate([[0], t["gt_id"]])
    return ids[dt_match]


def adversarial_oks(t, seed):
    """{image id: D x G matrix} of values that sit ON the decisions: exactly a threshold, 1 - 1e-10, 1.0, their neighbours, and
    all-equal rows; also the concatenated buffer."""
    rs = np.random.RandomState(seed)
    thr = np.asarray(t["thr"])
    pool = np.concatenate([thr, [1 - 1e-10, 1.0, np.nextafter(1 - 1e-10, 0), np.nextafter(1 - 1e-10, 1), 0.0, 0.49999], np.nextafter(thr, 0), np.nextafter(thr, 1)])
    by_image, flat = {}, np.zeros(int(t["oks_off"][-1]))
    for i, img in enumerate(t["img_ids"]):
        D, G = t["dt_off"][i + 1] - t["dt_off"][i], t["gt_off"][i + 1] - t["gt_off"][i]
        if D == 0 or G == 0:
            by_image[int(img)] = []
            continue
        m = rs.choice(pool[: rs.randint(1, len(pool) + 1)], (D, G))
        m[rs.rand(D) < 0.3] = rs.choice(pool)  # all-equal rows
        by_image[int(img)] = m
        flat[t["oks_off"][i]:t["oks_off"][i + 1]] = m.reshape(-1)
    return by_image, flat
