"""COCO keypoint AP / AR (OKS) evaluation -- the `eval_coco` step of `src/keypoints/bin/eval.py:52-65`.

The reference delegates this to pycocotools 2.0.7 (`COCO.loadRes` + `COCOeval(iouType="keypoints")`), a third-party
package that is NOT in this image and not under /root/reference.  This module restates its published algorithm
(cocoeval.py: computeOks, evaluateImg, accumulate, summarize; coco.py: loadRes for keypoint results) so that the
result lists of `keypoints.evaluation` can be scored without it.  PARITY UNPINNED: no golden vector from pycocotools
could be generated here; the tests check hand-derived cases only.

Two paths give the same numbers.  `evaluate()` is the host evaluator: nested Python loops with numpy inside, the yardstick.
`evaluate(device="cuda:0")` scores on the device: `pack_tables` (vectorised numpy: loadRes' area, _prepare's ignore flags, the per-image
stable sort by -score, the cut to maxDets) -> one host-to-device copy -> `hh_coco_evaluate` (csrc/coco_eval.hip: one launch, a workgroup
per image, OKS into LDS, one lane per (area range, threshold) for the matching walk) -> `accumulate_tables` (vectorised numpy on the
match tables copied back: one stable sort, cumulative sums, the precision envelope as a reversed running maximum, searchsorted).  The
match tables, ignore flags, `precision`, `recall` and `stats` of the two paths are identical (tests/test_coco_eval_budget_cpu.py,
tests/test_gpu_coco_eval.py); the OKS values agree to the rounding of exp and of the sum over joints, which the tests bound.
"""
from __future__ import annotations

import ctypes
import json
from collections import defaultdict
from itertools import chain, repeat
from operator import itemgetter

import numpy as np

from .. import _lib

KPT_OKS_SIGMAS = np.array([.26, .25, .25, .35, .35, .79, .79, .72, .72, .62, .62, 1.07, 1.07, .87, .87, .89, .89]) / 10.0
IOU_THRS = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
REC_THRS = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
MAX_DETS = [20]
AREA_RNG = [[0 ** 2, 1e5 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]
AREA_LBL = ["all", "medium", "large"]


def load_results(results: list[dict]) -> list[dict]:
    """COCO.loadRes for keypoint results: area / bbox from the keypoint extent, ids 1..N."""
    out = []
    for i, ann in enumerate(results):
        a = dict(ann)
        s = a["keypoints"]
        x, y = s[0::3], s[1::3]
        x0, x1, y0, y1 = np.min(x), np.max(x), np.min(y), np.max(y)
        a["area"] = float((x1 - x0) * (y1 - y0))
        a["id"] = i + 1
        a["bbox"] = [x0, y0, x1 - x0, y1 - y0]
        out.append(a)
    return out


class COCOKeypointsEval:
    """evaluate() + accumulate() + summarize() of COCOeval(iouType="keypoints"), person category only (useCats with one
    category).  `gt_annotations` = the "annotations" list of a person_keypoints json, `results` = list of result dicts."""

    def __init__(self, gt_annotations: list[dict], results: list[dict], img_ids=None, sigmas=KPT_OKS_SIGMAS):
        self.sigmas = np.asarray(sigmas, dtype=np.float64)
        dts = load_results(results)
        self._raw = (gt_annotations, results, img_ids)  # what pack_tables takes (the device path)
        self.img_ids = sorted(set(img_ids) if img_ids is not None else {d["image_id"] for d in dts})
        keep = set(self.img_ids)
        self._gts, self._dts = defaultdict(list), defaultdict(list)
        for g in gt_annotations:
            if g["image_id"] not in keep or g.get("category_id", 1) != 1:
                continue
            g = dict(g)
            g["ignore"] = bool(g.get("iscrowd", 0))               # cocoeval.py _prepare
            g["ignore"] = (g.get("num_keypoints", 0) == 0) or g["ignore"]
            self._gts[g["image_id"]].append(g)
        for d in dts:
            if d["image_id"] in keep and d.get("category_id", 1) == 1:
                self._dts[d["image_id"]].append(d)
        self.stats = None

    # ------------------------------------------------------------------ computeOks
    def _oks(self, img_id):
        gts, dts = self._gts[img_id], self._dts[img_id]
        inds = np.argsort([-d["score"] for d in dts], kind="mergesort")
        dts = [dts[i] for i in inds][: MAX_DETS[-1]]
        if len(gts) == 0 or len(dts) == 0:
            return []
        ious = np.zeros((len(dts), len(gts)))
        vars_ = (self.sigmas * 2) ** 2
        k = len(self.sigmas)
        for j, gt in enumerate(gts):
            g = np.array(gt["keypoints"], dtype=np.float64)
            xg, yg, vg = g[0::3], g[1::3], g[2::3]
            k1 = np.count_nonzero(vg > 0)
            bb = gt["bbox"]
            x0, x1 = bb[0] - bb[2], bb[0] + bb[2] * 2
            y0, y1 = bb[1] - bb[3], bb[1] + bb[3] * 2
            for i, dt in enumerate(dts):
                d = np.array(dt["keypoints"], dtype=np.float64)
                xd, yd = d[0::3], d[1::3]
                if k1 > 0:
                    dx, dy = xd - xg, yd - yg
                else:  # no labelled joint: distance to the doubled box
                    z = np.zeros(k)
                    dx = np.max((z, x0 - xd), axis=0) + np.max((z, xd - x1), axis=0)
                    dy = np.max((z, y0 - yd), axis=0) + np.max((z, yd - y1), axis=0)
                e = (dx ** 2 + dy ** 2) / vars_ / (gt["area"] + np.spacing(1)) / 2
                if k1 > 0:
                    e = e[vg > 0]
                ious[i, j] = np.sum(np.exp(-e)) / e.shape[0]
        return ious

    # ------------------------------------------------------------------ evaluateImg
    def _evaluate_img(self, img_id, ious, a_rng, max_det):
        gt, dt = self._gts[img_id], self._dts[img_id]
        if len(gt) == 0 and len(dt) == 0:
            return None
        g_ign = [1 if (g["ignore"] or g["area"] < a_rng[0] or g["area"] > a_rng[1]) else 0 for g in gt]
        gtind = np.argsort(g_ign, kind="mergesort")
        gt = [gt[i] for i in gtind]
        dtind = np.argsort([-d["score"] for d in dt], kind="mergesort")
        dt = [dt[i] for i in dtind[:max_det]]
        iscrowd = [int(g.get("iscrowd", 0)) for g in gt]
        ious = ious[:, gtind] if len(ious) > 0 else ious
        T, G, D = len(IOU_THRS), len(gt), len(dt)
        gtm, dtm = np.zeros((T, G)), np.zeros((T, D))
        gt_ig = np.array([g_ign[i] for i in gtind])
        dt_ig = np.zeros((T, D))
        if len(ious) != 0:
            for tind, t in enumerate(IOU_THRS):
                for dind, d in enumerate(dt):
                    iou = min([t, 1 - 1e-10])
                    m = -1
                    for gind in range(G):
                        if gtm[tind, gind] > 0 and not iscrowd[gind]:
                            continue
                        if m > -1 and gt_ig[m] == 0 and gt_ig[gind] == 1:
                            break
                        if ious[dind, gind] < iou:
                            continue
                        iou = ious[dind, gind]
                        m = gind
                    if m == -1:
                        continue
                    dt_ig[tind, dind] = gt_ig[m]
                    dtm[tind, dind] = gt[m]["id"]
                    gtm[tind, m] = d["id"]
        a = np.array([d["area"] < a_rng[0] or d["area"] > a_rng[1] for d in dt]).reshape((1, len(dt)))
        dt_ig = np.logical_or(dt_ig, np.logical_and(dtm == 0, np.repeat(a, T, 0)))
        return {"dtMatches": dtm, "dtScores": [d["score"] for d in dt], "gtIgnore": gt_ig, "dtIgnore": dt_ig}

    # ------------------------------------------------------------------ evaluate + accumulate + summarize
    def evaluate(self, device=None):
        """device=None: the host evaluator below.  A device string ("cuda:0"): the same numbers from `evaluate_device`."""
        if device is not None:
            self.precision, self.recall, self.stats = evaluate_device(self._raw[0], self._raw[1], device, self._raw[2], self.sigmas)
            return self.stats
        ious = {i: self._oks(i) for i in self.img_ids}
        max_det = MAX_DETS[-1]
        T, R, A, M = len(IOU_THRS), len(REC_THRS), len(AREA_RNG), len(MAX_DETS)
        precision, recall = -np.ones((T, R, A, M)), -np.ones((T, A, M))
        for a, a_rng in enumerate(AREA_RNG):
            E = [e for e in (self._evaluate_img(i, ious[i], a_rng, max_det) for i in self.img_ids) if e is not None]
            for m, md in enumerate(MAX_DETS):
                if len(E) == 0:
                    continue
                dt_scores = np.concatenate([e["dtScores"][0:md] for e in E])
                inds = np.argsort(-dt_scores, kind="mergesort")
                dtm = np.concatenate([e["dtMatches"][:, 0:md] for e in E], axis=1)[:, inds]
                dt_ig = np.concatenate([e["dtIgnore"][:, 0:md] for e in E], axis=1)[:, inds]
                gt_ig = np.concatenate([e["gtIgnore"] for e in E])
                npig = np.count_nonzero(gt_ig == 0)
                if npig == 0:
                    continue
                tps = np.logical_and(dtm, np.logical_not(dt_ig))
                fps = np.logical_and(np.logical_not(dtm), np.logical_not(dt_ig))
                tp_sum = np.cumsum(tps, axis=1).astype(dtype=float)
                fp_sum = np.cumsum(fps, axis=1).astype(dtype=float)
                for t, (tp, fp) in enumerate(zip(tp_sum, fp_sum)):
                    nd = len(tp)
                    rc = tp / npig
                    pr = tp / (fp + tp + np.spacing(1))
                    q = np.zeros((R,))
                    recall[t, a, m] = rc[-1] if nd else 0
                    pr = pr.tolist()
                    q = q.tolist()
                    for i in range(nd - 1, 0, -1):  # precision envelope
                        if pr[i] > pr[i - 1]:
                            pr[i - 1] = pr[i]
                    inds_r = np.searchsorted(rc, REC_THRS, side="left")
                    for ri, pi in enumerate(inds_r):
                        if pi >= nd:
                            break
                        q[ri] = pr[pi]
                    precision[t, :, a, m] = np.array(q)
        self.precision, self.recall = precision, recall

        def summ(ap, iou_thr=None, area="all"):
            aind = AREA_LBL.index(area)
            s = precision[:, :, aind, 0] if ap else recall[:, aind, 0]
            if iou_thr is not None:
                s = s[np.where(np.isclose(iou_thr, IOU_THRS))[0]]
            return -1.0 if len(s[s > -1]) == 0 else float(np.mean(s[s > -1]))

        self.stats = np.array([summ(1), summ(1, .5), summ(1, .75), summ(1, area="medium"), summ(1, area="large"),
                               summ(0), summ(0, .5), summ(0, .75), summ(0, area="medium"), summ(0, area="large")])
        return self.stats

    def summary_text(self) -> str:
        names = ["AP", "AP .5", "AP .75", "AP (M)", "AP (L)", "AR", "AR .5", "AR .75", "AR (M)", "AR (L)"]
        return "\n".join(f" {n:7s} = {v:0.3f}" for n, v in zip(names, self.stats))


def eval_coco(annots_path: str, results_path: str, device=None) -> np.ndarray:
    """bin/eval.py:52-65 with files: person_keypoints_*.json + the results json written by the evaluation loop.
    `device`: None = the host evaluator, a device string = the device path (COCOKeypointsEval.evaluate)."""
    with open(annots_path) as f:
        gt = json.load(f)["annotations"]
    with open(results_path) as f:
        res = json.load(f)
    ev = COCOKeypointsEval(gt, res)
    ev.evaluate(device)
    print(ev.summary_text())
    return ev.stats


# ---------------------------------------------------------------------- the device path
_TABLE_FIELDS = ("dt_off", "gt_off", "oks_off", "dt_xy", "dt_score", "dt_area", "gt_xyv", "gt_area", "gt_bbox", "gt_flags", "vars", "area_rng", "thr")
GT_IGNORE, GT_CROWD = _lib.const("COCO_GT_IGNORE"), _lib.const("COCO_GT_CROWD")


CocoTables = _lib.struct_ctype("hh_coco_tables")  # 13 addresses, the six counts


def _column(dicts, key, default=None):
    """[d[key] for d in dicts] (or d.get(key, default)) without an interpreter loop over the rows."""
    if default is None:
        return list(map(itemgetter(key), dicts))
    return list(map(dict.get, dicts, repeat(key), repeat(default)))


def _rows(dicts, key, width):
    """np.array([d[key] for d in dicts], float64) for rows of `width` numbers, read through one flat iterator (several times faster
    than numpy's nested-list conversion, and again no interpreter loop over the rows)."""
    col = _column(dicts, key)
    if any(map(lambda n: n != width, set(map(len, col)))):
        raise ValueError(f"every '{key}' must have {width} entries")
    return np.fromiter(chain.from_iterable(col), np.float64, count=len(col) * width).reshape(len(col), width)


def pack_tables(gt_annotations: list[dict], results: list[dict], img_ids=None, sigmas=KPT_OKS_SIGMAS, max_det: int = MAX_DETS[-1]) -> dict:
    """The tables `hh_coco_evaluate` reads, as numpy arrays: what COCOKeypointsEval.__init__ (load_results' area and bbox, _prepare's
    ignore flags, the image / category filter) and the head of _oks / _evaluate_img (per image: the stable sort by -score, the cut to
    `max_det`) produce, formed with array operations only.  Ground truths keep their annotation order within an image.  Besides the
    tables of hh_coco_tables: `img_ids` (sorted), `dt_id` / `gt_id` (the ids the host evaluator reports: result index + 1, annotation
    id) and `dt_bbox`."""
    sig = np.asarray(sigmas, dtype=np.float64)
    K = len(sig)
    n_res = len(results)
    kp = _rows(results, "keypoints", K * 3)
    d_img = np.asarray(_column(results, "image_id"), dtype=np.int64).reshape(n_res)
    d_cat = np.asarray(_column(results, "category_id", 1), dtype=np.int64).reshape(n_res)
    score = np.asarray(_column(results, "score"), dtype=np.float64).reshape(n_res)
    ids = np.unique(np.asarray(list(img_ids), dtype=np.int64)) if img_ids is not None else np.unique(d_img)
    n_img = len(ids)

    def image_index(img):  # row of `ids`, -1 where the image is not evaluated
        pos = np.searchsorted(ids, img)
        ok = (pos < n_img) & (ids[np.minimum(pos, max(n_img - 1, 0))] == img) if n_img else np.zeros(len(img), bool)
        return np.where(ok, pos, -1)

    d_at = image_index(d_img)
    keep = np.nonzero((d_at >= 0) & (d_cat == 1))[0]
    order = keep[np.lexsort((-score[keep], d_at[keep]))]  # by image, then by -score; stable: ties keep the order of `results`
    counts = np.bincount(d_at[order], minlength=n_img) if n_img else np.zeros(0, np.int64)
    starts = np.concatenate([[0], np.cumsum(counts)])
    rank = np.arange(len(order)) - starts[d_at[order]] if len(order) else np.zeros(0, np.int64)
    order = order[rank < max_det]                         # dts[:max_det]
    D = np.minimum(counts, max_det)
    x, y = kp[order, 0::3], kp[order, 1::3]
    if len(order):
        x0, x1, y0, y1 = x.min(1), x.max(1), y.min(1), y.max(1)
    else:
        x0 = x1 = y0 = y1 = np.zeros(0)
    dt_area = (x1 - x0) * (y1 - y0)

    n_gt = len(gt_annotations)
    g_img = np.asarray(_column(gt_annotations, "image_id"), dtype=np.int64).reshape(n_gt)
    g_cat = np.asarray(_column(gt_annotations, "category_id", 1), dtype=np.int64).reshape(n_gt)
    g_at = image_index(g_img)
    gkeep = np.nonzero((g_at >= 0) & (g_cat == 1))[0]
    gorder = gkeep[np.argsort(g_at[gkeep], kind="stable")]
    G = np.bincount(g_at[gorder], minlength=n_img) if n_img else np.zeros(0, np.int64)
    crowd = np.asarray(_column(gt_annotations, "iscrowd", 0), dtype=np.int64).reshape(n_gt)[gorder] != 0
    nkp = np.asarray(_column(gt_annotations, "num_keypoints", 0), dtype=np.int64).reshape(n_gt)[gorder]
    gkp = _rows(gt_annotations, "keypoints", K * 3)[gorder]
    g_area = np.asarray(_column(gt_annotations, "area"), dtype=np.float64).reshape(n_gt)[gorder]
    g_bbox = _rows(gt_annotations, "bbox", 4)[gorder]
    g_id = np.asarray(_column(gt_annotations, "id"), dtype=np.int64).reshape(n_gt)[gorder]
    flags = (((nkp == 0) | crowd) * GT_IGNORE + crowd * GT_CROWD).astype(np.uint8)

    c = np.ascontiguousarray
    return {
        "dt_off": np.concatenate([[0], np.cumsum(D)]).astype(np.int32), "gt_off": np.concatenate([[0], np.cumsum(G)]).astype(np.int32),
        "oks_off": np.concatenate([[0], np.cumsum(D * G)]).astype(np.int64),
        "dt_xy": c(np.stack([x, y], -1).reshape(len(order), K, 2)), "dt_score": c(score[order]), "dt_area": c(dt_area),
        "gt_xyv": c(gkp.reshape(len(gorder), K, 3)), "gt_area": c(g_area), "gt_bbox": c(g_bbox), "gt_flags": flags,
        "vars": (sig * 2) ** 2, "area_rng": np.asarray(AREA_RNG, dtype=np.float64), "thr": np.asarray(IOU_THRS, dtype=np.float64),
        "img_ids": ids, "dt_id": order + 1, "gt_id": g_id, "dt_bbox": np.stack([x0, y0, x1 - x0, y1 - y0], -1),
    }


def tables_struct(tables: dict, address_of) -> CocoTables:
    """hh_coco_tables over `tables`; address_of(name) gives each table's address (host or device)."""
    t = CocoTables()
    for n in _TABLE_FIELDS:
        setattr(t, n, address_of(n))
    t.I, t.N, t.M = len(tables["dt_off"]) - 1, len(tables["dt_score"]), len(tables["gt_area"])
    t.K, t.A, t.T = len(tables["vars"]), len(tables["area_rng"]), len(tables["thr"])
    return t


def host_struct(tables: dict) -> CocoTables:
    """The caller's host copy, for validation and for hh_coco_evaluate_host.  An empty table still gets a non-null address."""
    return tables_struct(tables, lambda n: tables[n].ctypes.data or ctypes.addressof(_EMPTY))


_EMPTY = ctypes.c_double(0.0)


def blob_layout(tables: dict):
    """All tables of hh_coco_tables in ONE byte buffer (each 8-byte aligned), so that they reach the device in one copy:
    (uint8 array, {name: offset})."""
    offs, at = {}, 0
    for n in _TABLE_FIELDS:
        offs[n] = at
        at += (tables[n].nbytes + 7) // 8 * 8
    blob = np.zeros(max(at, 8), np.uint8)
    for n in _TABLE_FIELDS:
        blob[offs[n]:offs[n] + tables[n].nbytes] = tables[n].reshape(-1).view(np.uint8)
    return blob, offs


def match_tables_device(tables: dict, device):
    """pack -> one copy -> hh_coco_evaluate -> the three match tables back as numpy: dt_match int32 [A,T,N] (row of the ground-truth
    table + 1, 0 = unmatched), dt_ignore bool [A,T,N], gt_ignore bool [A,M]."""
    import torch
    lib = _lib.load()
    A, T, N, M = len(tables["area_rng"]), len(tables["thr"]), len(tables["dt_score"]), len(tables["gt_area"])
    blob, offs = blob_layout(tables)
    dev_blob = torch.from_numpy(blob).to(device)
    n_match = A * T * N
    out = torch.empty(n_match * 4 + n_match + A * M + 8, dtype=torch.uint8, device=device)  # dt_match | dt_ignore | gt_ignore
    dev = tables_struct(tables, lambda n: dev_blob.data_ptr() + offs[n])
    host = host_struct(tables)
    _lib.launch(dev_blob.device, lib.hh_coco_evaluate, ctypes.byref(dev), ctypes.byref(host), out.data_ptr(), out.data_ptr() + n_match * 4,
                out.data_ptr() + n_match * 5)
    back = out.cpu().numpy()
    dt_match = back[:n_match * 4].view(np.int32).reshape(A, T, N)
    dt_ignore = back[n_match * 4:n_match * 5].reshape(A, T, N) != 0
    gt_ignore = back[n_match * 5:n_match * 5 + A * M].reshape(A, M) != 0
    return dt_match, dt_ignore, gt_ignore


def match_tables_host(tables: dict, oks_in=None, want_oks: bool = False):
    """The same through hh_coco_evaluate_host (csrc/coco_eval_math.h compiled for the host): (dt_match, dt_ignore, gt_ignore[, oks]).
    `oks_in`: a concatenated float64 buffer to match on instead of computing it (the host form of hh_coco_match)."""
    lib = _lib.load()
    A, T, N, M = len(tables["area_rng"]), len(tables["thr"]), len(tables["dt_score"]), len(tables["gt_area"])
    dt_match, dt_ignore, gt_ignore = np.zeros(A * T * N + 1, np.int32), np.zeros(A * T * N + 1, np.uint8), np.zeros(A * M + 1, np.uint8)
    oks = np.zeros(int(tables["oks_off"][-1]) + 1, np.float64) if want_oks else None
    if oks_in is not None:
        oks_in = np.ascontiguousarray(oks_in, dtype=np.float64)
        assert oks_in.size >= int(tables["oks_off"][-1])
    host = host_struct(tables)
    p_in = None if oks_in is None else (oks_in.ctypes.data or ctypes.addressof(_EMPTY))
    _lib.check(lib.hh_coco_evaluate_host(ctypes.byref(host), p_in, oks.ctypes.data if oks is not None else None, dt_match.ctypes.data,
                                         dt_ignore.ctypes.data, gt_ignore.ctypes.data))
    res = (dt_match[:-1].reshape(A, T, N), dt_ignore[:-1].reshape(A, T, N) != 0, gt_ignore[:-1].reshape(A, M) != 0)
    return res + (oks[:-1],) if want_oks else res


def accumulate_tables(dt_score, dt_match, dt_ignore, gt_ignore, rec_thrs=REC_THRS):
    """COCOeval.accumulate on the match tables, with array operations: -> precision [T,R,A,1], recall [T,A,1], bit-identical to the
    loops of COCOKeypointsEval.evaluate.  The images' detections are already concatenated in image order, so ONE stable sort by -score
    serves every area range; cumulative TP / FP counts are integers; the two divisions are numpy's, in the host's expressions; the
    precision envelope is a running maximum from the right."""
    A, T, N = dt_match.shape
    R = len(rec_thrs)
    precision, recall = -np.ones((T, R, A, 1)), -np.ones((T, A, 1))
    inds = np.argsort(-np.asarray(dt_score), kind="mergesort")
    dtm, dt_ig = dt_match[:, :, inds] != 0, np.asarray(dt_ignore, bool)[:, :, inds]
    tp_sum = np.cumsum(dtm & ~dt_ig, axis=2).astype(dtype=float)
    fp_sum = np.cumsum(~dtm & ~dt_ig, axis=2).astype(dtype=float)
    npig = np.count_nonzero(~np.asarray(gt_ignore, bool), axis=1)
    for a in range(A):
        if npig[a] == 0:  # (covers the host's `len(E) == 0`: no image with a ground truth or a detection)
            continue
        tp, fp = tp_sum[a], fp_sum[a]
        rc = tp / npig[a]
        pr = tp / (fp + tp + np.spacing(1))
        pr = np.maximum.accumulate(pr[:, ::-1], axis=1)[:, ::-1]
        recall[:, a, 0] = rc[:, -1] if N else 0
        for t in range(T):  # (A * T searchsorted calls, none over detections)
            at = np.searchsorted(rc[t], rec_thrs, side="left")
            q = np.zeros(R)
            q[at < N] = pr[t, at[at < N]]
            precision[t, :, a, 0] = q
    return precision, recall


def summarize(precision, recall) -> np.ndarray:
    """COCOeval.summarize for keypoints: the ten numbers of `stats`, in evaluate()'s expressions."""
    def summ(ap, iou_thr=None, area="all"):
        aind = AREA_LBL.index(area)
        s = precision[:, :, aind, 0] if ap else recall[:, aind, 0]
        if iou_thr is not None:
            s = s[np.where(np.isclose(iou_thr, IOU_THRS))[0]]
        return -1.0 if len(s[s > -1]) == 0 else float(np.mean(s[s > -1]))

    return np.array([summ(1), summ(1, .5), summ(1, .75), summ(1, area="medium"), summ(1, area="large"),
                     summ(0), summ(0, .5), summ(0, .75), summ(0, area="medium"), summ(0, area="large")])


def evaluate_device(gt_annotations, results, device, img_ids=None, sigmas=KPT_OKS_SIGMAS, timings: dict | None = None):
    """pack_tables -> hh_coco_evaluate on `device` -> accumulate_tables -> summarize: (precision, recall, stats), the arrays
    COCOKeypointsEval.evaluate() leaves.  `timings`, if given, receives the seconds of the three parts."""
    import time
    t0 = time.perf_counter()
    tables = pack_tables(gt_annotations, results, img_ids, sigmas)
    t1 = time.perf_counter()
    dt_match, dt_ignore, gt_ignore = match_tables_device(tables, device)
    t2 = time.perf_counter()
    precision, recall = accumulate_tables(tables["dt_score"], dt_match, dt_ignore, gt_ignore)
    stats = summarize(precision, recall)
    if timings is not None:
        timings.update(pack=t1 - t0, copy_launch_copy=t2 - t1, accumulate=time.perf_counter() - t2)
    return precision, recall, stats
