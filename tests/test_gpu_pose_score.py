"""Per-image OKS / PCKh on the GPU (hh_pose_score_batch; keypoints/pose_score.py) against the host twin on the lattice of
tests/pose_score_budget.py in both prediction forms, and end to end through InferenceKeypointsModel.infer_images(score=...) and
evaluate_images(image_scores=True) at 128 x 128 on synthetic weights.

Device against host twin: statuses, match indices, PCKh values and image values exact (the lattice is separated); per-joint terms within
the two exp bounds (OCML 1 ulp + glibc 1 ulp), object OKS within the derived budget.  Worst ratios measured: profiles/pose_score.md."""
import importlib

import numpy as np
import pytest
import torch

import pose_score_budget as lat
from conftest import PKG

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FIELDS = ("kpts_coords", "kpts_scores", "kpts_tags", "obj_scores")
ULPS = 2 * lat.ULP_EXP_TEST


@pytest.fixture(scope="module")
def ps(pkg):
    return importlib.import_module(PKG + ".keypoints.pose_score")


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))


def run_both(ps, c, t, form, decode=None, preds=None):
    decode = t["decode"] if decode is None else decode
    preds = t["preds"] if preds is None else preds
    kw = dict(metric=c["metric"], variances=c["variances"], alpha=c["alpha"])
    if form == "decode":
        host = ps.score_host(t["targets"], decode=decode, inv_affine=t["inv_affine"], **kw)
        got = ps.score_device(t["targets"], decode=tuple(dev(a) for a in decode), inv_affine=t["inv_affine"], **kw).to_host()
    else:
        host = ps.score_host(t["targets"], preds=preds, **kw)
        got = ps.score_device(t["targets"], preds=preds, device=DEV, **kw).to_host()
    return host, got


@pytest.mark.parametrize("form", ["decode", "f64"])
@pytest.mark.parametrize("name", lat.LATTICE)
def test_device_equals_host_twin(ps, name, form):
    c, t, r = lat.case(name)
    host, got = run_both(ps, c, t, form)
    assert np.array_equal(got["status"], host["status"]) and (got["status"] == 0).all()
    assert np.array_equal(got["match"], host["match"]) and np.array_equal(got["match"], r["match"])
    assert np.array_equal(got["kpt"] < 0, host["kpt"] < 0)
    if c["metric"] == "pckh":
        assert _same_bits(got["kpt"], host["kpt"]) and _same_bits(got["obj"], host["obj"])
    else:
        ratio_k = np.abs(got["kpt"] - host["kpt"]) / (ULPS * np.spacing(np.abs(host["kpt"])))
        ratio_o = np.abs(got["obj"] - host["obj"]) / lat.oks_budget(host["kpt"], ULPS)
        print(f"{name}/{form}: worst ratio term {ratio_k.max(initial=0):.3f} object {ratio_o.max(initial=0):.3f}")
        assert (ratio_k <= 1).all() and (ratio_o <= 1).all()
    assert _same_bits(got["value"], host["value"])


def test_device_at_the_maxima(ps):
    """P = 64 people of K = 64 joints in the F64 form: 72 KB of dynamic LDS, above the 64 KB a launch gets without the function attribute.
    D is formed by the same text in the same order on both sides, so the match indices are equal without a separation condition."""
    rs = np.random.RandomState(21)
    P, K, T = 64, 64, 5
    xyv = np.concatenate([np.round(rs.uniform(0, 400, (T, K, 2))), rs.randint(0, 3, (T, K, 1))], -1)
    xyv[:, 0, 2] = 2
    xy = rs.uniform(0, 400, (P, K, 2))
    xy[60:64] = xyv[:4, :, :2] + rs.normal(0, 3.0, (4, K, 2))  # the last rows of the LDS array are the ones that match
    preds = [(xy, np.round(rs.uniform(0.1, 0.9, P), 1))]      # (equal scores happen)
    targets = ps.make_targets(xyv, t_area=np.full(T, 9000.0))
    var = rs.uniform(0.002, 0.04, K)
    assert ps.config()["lds_bytes_max"] > 64 * 1024
    host = ps.score_host(targets, preds=preds, variances=var)
    got = ps.score_device(targets, preds=preds, variances=var, device=DEV).to_host()
    assert (host["status"] == 0).all() and np.array_equal(got["status"], host["status"]) and np.array_equal(got["match"], host["match"])
    assert host["match"][:4].tolist() == [60, 61, 62, 63] and np.array_equal(got["kpt"] < 0, host["kpt"] < 0)
    budget = lat.oks_budget(host["kpt"], ULPS)
    assert (np.abs(got["kpt"] - host["kpt"]) <= ULPS * np.spacing(np.abs(host["kpt"]))).all() and (np.abs(got["obj"] - host["obj"]) <= budget).all()
    scaled = host["obj"] * 1000.0
    assert not (np.abs(scaled - (np.floor(scaled) + 0.5)) <= 1000.0 * budget + lat.U * scaled).any()  # (seeded: no rounding can flip)
    assert _same_bits(got["value"], host["value"]) and 0.0 < host["value"][0] < 1.0


def test_device_status_bits(ps):
    c, t, r = lat.case("k17_mixed")
    joints = t["decode"][0].copy()
    joints[1, 29, 16, 1] = np.inf   # the last joint of the last person
    joints[3, 0, 0, 0] = np.nan     # the fallback image
    host, got = run_both(ps, c, t, "decode", decode=(joints,) + t["decode"][1:])
    assert got["status"].tolist() == [0, ps.NONFINITE, 0, ps.NONFINITE, 0] == host["status"].tolist()
    assert np.array_equal(got["match"], host["match"]) and np.array_equal(np.isnan(got["obj"]), np.isnan(host["obj"]))
    assert np.array_equal(np.isnan(got["kpt"]), np.isnan(host["kpt"])) and np.isnan(got["value"][[1, 3]]).all()
    assert _same_bits(got["value"][[0, 2, 4]], r["value"][[0, 2, 4]])
    preds = [(xy.copy(), s.copy()) for xy, s in t["preds"]]
    preds[0] = (np.zeros((0, 17, 2)), np.zeros(0))
    host, got = run_both(ps, c, t, "f64", preds=preds)
    assert got["status"].tolist() == [ps.NO_PRED, 0, 0, 0, 0] == host["status"].tolist() and np.isnan(got["value"][0]) and got["match"][0] == -1


def test_device_refuses_before_any_launch(ps, pkg):
    targets, preds = lat.over_the_maxima("targets")
    with pytest.raises(pkg._lib.HHError, match="image 0 has 129 targets, over HH_POSE_MAX_T"):
        ps.score_device(targets, preds=preds, device=DEV)
    targets, preds = lat.over_the_maxima("predictions")
    with pytest.raises(pkg._lib.HHError, match="image 0 has 65 predictions, over HH_POSE_MAX_P"):
        ps.score_device(targets, preds=preds, device=DEV)
    empty = ps.make_targets(np.zeros((0, 17, 3)), t_off=[0])
    assert ps.score_device(empty, preds=[], device=DEV).to_host()["value"].shape == (0,)


@pytest.fixture(scope="module")
def model(pkg):
    net = pkg.HigherHRNet(17, 32)
    net.load_state_dict({k: torch.from_numpy(pkg.synth.synth_param(k, v.shape, 3)) for k, v in net.state_dict().items()})
    return pkg.InferenceKeypointsModel(net.to(DEV).eval(), det_thr=0.05, tag_thr=0.5, use_flip=False, input_size=128, device=DEV)


@pytest.fixture(scope="module")
def scene(model):
    """Five tiny images of two shapes, a plain run over them, and annotations made from that run's own predictions: every second person
    becomes an annotated object (coordinates rounded and shifted, some joints unlabelled), plus one object nobody predicted."""
    rs = np.random.RandomState(11)
    images = [rs.randint(0, 255, s).astype(np.uint8) for s in ((128, 128, 3), (96, 160, 3), (128, 128, 3), (160, 96, 3), (128, 128, 3))]
    plain = model.infer_images(images, max_batch=4)
    annots = []
    for i, res in enumerate(plain):
        objs = []
        for p in range(0, len(res.kpts_coords), 2):
            v = rs.randint(0, 3, 17)
            v[rs.randint(17)] = 2
            xy = np.where(v[:, None] > 0, np.round(res.kpts_coords[p].astype(np.float64)) + rs.randint(-3, 4, (17, 2)), 0)
            x0, y0, x1, y1 = xy[v > 0, 0].min(), xy[v > 0, 1].min(), xy[v > 0, 0].max() + 20, xy[v > 0, 1].max() + 30
            objs.append({"image_id": 100 + i, "keypoints": np.concatenate([xy, v[:, None]], 1).astype(int).reshape(-1).tolist(),
                         "segmentation": [[x0, y0, x1, y0, x1, y1, x0, y1]], "head_xyxy": (0, 0, 6 + p, 8)})
        objs.append({"image_id": 100 + i, "keypoints": [0] * 51, "segmentation": {"counts": [1], "size": [1, 1]}})  # unlabelled: not a target
        annots.append(objs)
    annots[2] = None   # not scored
    annots[4] = [annots[4][-1]]  # an annotation without a labelled object: -1
    return images, plain, annots


def check_scored(ps, scored, plain, annots):
    flips = 0
    for i, (a, b) in enumerate(zip(plain, scored)):
        for f in FIELDS:  # the results themselves are what they are without score=
            assert np.array_equal(getattr(a, f), getattr(b, f)), f
        if annots[i] is None:
            assert b.oks is None and b.object_oks is None and b.kpt_oks is None and b.target_matches is None
            continue
        T = len(ps.labelled_objects(annots[i]))
        later = type(a)(a.raw_image, annots[i], None, a.kpts_coords, a.kpts_scores, a.kpts_tags, a.obj_scores, a.det_thr, a.tag_thr)
        value = later.calculate_OKS()  # hh_pose_score_host on the copied-back arrays, the F64 form
        assert b.calculate_OKS() == b.oks  # (the stored value)
        assert b.object_oks.shape == (T,) and b.kpt_oks.shape == (T, 17) and b.target_matches.shape == (T,) and b.target_matches.dtype == np.int32
        if T == 0:
            assert b.oks == -1 == value
            continue
        assert np.array_equal(b.target_matches, later.target_matches)
        budget = lat.oks_budget(later.kpt_oks, ULPS)
        assert (np.abs(b.object_oks - later.object_oks) <= budget).all() and np.array_equal(b.kpt_oks < 0, later.kpt_oks < 0)
        scaled = later.object_oks * 1000.0
        unsafe = int((np.abs(scaled - (np.floor(scaled) + 0.5)) <= 1000.0 * budget + lat.U * scaled).sum())  # a rounding that may flip
        flips += unsafe
        assert unsafe == 0, "the seeded scene has an object OKS within its budget of a rounding boundary: choose another seed"
        assert b.oks == value  # equal rounded objects, summed in the same order
    return flips


def test_infer_images_score_oks(ps, model, scene):
    images, plain, annots = scene
    scored = model.infer_images(images, annots=annots, max_batch=4, score="oks")
    flips = check_scored(ps, scored, plain, annots)
    print("people:", [len(r.kpts_coords) for r in plain], "targets:", [None if a is None else len(ps.labelled_objects(a)) for a in annots],
          "oks:", [r.oks for r in scored], "roundings within budget of a half:", flips)
    with pytest.raises(ValueError, match="score must be None, 'oks' or 'pckh'"):
        model.infer_images(images[:1], annots=annots[:1], score="iou")
    with pytest.raises(ValueError, match="run-length"):
        model.infer_images(images[:1], annots=[[dict(annots[0][0], segmentation={"counts": [1], "size": [1, 1]})]], score="oks")
    # refused before anything is enqueued: the COCO constants belong to 17 keypoints; at most 64 people
    keep = model._parser.num_kpts, model._parser.max_num_people
    try:
        model._parser.num_kpts = 16
        with pytest.raises(ValueError, match="17 COCO keypoints, not of 16"):
            model.infer_images(images[:1], annots=annots[:1], score="oks")
        model._parser.num_kpts, model._parser.max_num_people = keep[0], 65
        with pytest.raises(ValueError, match="at most HH_POSE_MAX_P"):
            model.infer_images(images[:1], annots=annots[:1], score="oks")
    finally:
        model._parser.num_kpts, model._parser.max_num_people = keep
    # batches of different target counts share their pinned result buffers: the output array's size does not follow T
    before = len(model._out_ring)
    for n in (1, 2, 3):
        fewer = [None if a is None else a[:n] + a[-1:] for a in annots]
        model.infer_images(images, annots=fewer, max_batch=4, score="oks")
    assert len(model._out_ring) == before
    # an un-annotated batch launches nothing and changes nothing
    none = model.infer_images(images[:2], annots=[None, None], max_batch=4, score="oks")
    assert all(r.oks is None for r in none) and all(np.array_equal(a.kpts_coords, b.kpts_coords) for a, b in zip(plain, none))


def test_infer_images_score_behind_tracker_and_scales(ps, pkg, model, scene):
    images, plain, annots = scene
    tk = importlib.import_module(PKG + ".keypoints.tracking")
    same = [0, 2, 4]  # the 128 x 128 frames
    tracked = model.infer_images([images[i] for i in same], annots=[annots[i] for i in same], max_batch=4, tracker=tk.PoseTracker(device=DEV), score="oks")
    check_scored(ps, tracked, [plain[i] for i in same], [annots[i] for i in same])
    assert all(r.track_ids is not None for r in tracked)
    scales = (0.5, 1.0)
    multi_plain = model.infer_images(images[:2], max_batch=4, scales=scales)
    multi = model.infer_images(images[:2], annots=annots[:2], max_batch=4, scales=scales, score="oks")
    check_scored(ps, multi, multi_plain, annots[:2])


def test_infer_images_score_pckh(ps, model, scene):
    images, plain, annots = scene
    scored = model.infer_images(images[:2], annots=annots[:2], max_batch=4, score="pckh")
    for a, b, annot in zip(plain, scored, annots):
        assert b.oks is None and all(np.array_equal(getattr(a, f), getattr(b, f)) for f in FIELDS)
        tg = ps.pack_targets([annot], "pckh")
        host = ps.score_host(tg, preds=[(a.kpts_coords, a.obj_scores)], metric="pckh")
        assert b.pckh == host["value"][0] and np.array_equal(b.object_pckh, host["obj"]) and np.array_equal(b.kpt_pckh, host["kpt"])
        assert np.array_equal(b.target_matches, host["match"])


def test_evaluate_images_image_scores(ps, pkg, model, scene):
    images, plain, annots = scene
    ev = importlib.import_module(PKG + ".keypoints.evaluation")
    ids = [100 + i for i in range(len(images))]
    gt = [o for a in annots if a is not None for o in a if isinstance(o["segmentation"], list)]
    packed, by_image, joint_mean = ev.evaluate_images(model, images, ids, batch=4, gt_annotations=gt, image_scores=True)
    assert packed == ev.evaluate_images(model, images, ids, batch=4)
    scored = model.infer_images(images, annots=[[o for o in gt if o["image_id"] == i] for i in ids], max_batch=4, score="oks")
    assert by_image == {i: r.oks for i, r in zip(ids, scored)} and by_image[102] == -1 and by_image[104] == -1
    terms = np.concatenate([r.kpt_oks for r in scored])
    lab = terms >= 0
    want = np.where(lab, terms, 0).sum(0) / lab.sum(0)
    assert joint_mean.shape == (17,) and np.allclose(joint_mean, want, rtol=1e-14, atol=0, equal_nan=True)
    with pytest.raises(ValueError, match="needs gt_annotations"):
        ev.evaluate_images(model, images, ids, image_scores=True)
