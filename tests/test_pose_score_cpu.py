"""Per-image OKS / PCKh against annotations, without a GPU: the restatement (tests/pose_score_ref.py) against the fixture made by the
reference's own functions (tests/golden/pose_score.npz, tools/make_pose_score_golden.py), the host twin (hh_pose_score_host: the
kernel's text compiled for the host) against the restatement in both prediction forms, the planted defects, the refusals, the polygon
area.  Budgets and separation conditions: tests/pose_score_budget.py.

Worst budget ratios measured on the lattice (|difference| / budget, profiles/pose_score.md): restatement against the reference 0.091
(object OKS), host twin against the restatement 0.20 (per-joint term) and 0.146 (object OKS); every match index, every PCKh value and
every image value exact."""
import importlib
import json
import os

import numpy as np
import pytest

import pose_score_budget as lat
import pose_score_ref as ref
from conftest import PKG, REPO

GOLDEN = os.path.join(REPO, "tests", "golden", "pose_score.npz")


@pytest.fixture(scope="module")
def ps(pkg):
    return importlib.import_module(PKG + ".keypoints.pose_score")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))


def _term_bound(kpt):
    return (lat.ULP_EXP_HOST + lat.ULP_EXP_TEST) * np.spacing(np.abs(kpt))


def check_against(c, t, want, got, exact_terms: bool, label: str):
    """`got` (an implementation of the header) against `want` (the restatement) on a separated case: statuses, match indices and
    unlabelled marks equal; terms within exp's bound; objects within the budget; PCKh exact; the image value exact (equal rounded
    objects summed in the same order)."""
    assert np.array_equal(got["status"], want["status"]), label
    assert np.array_equal(got["match"], want["match"]), label
    assert np.array_equal(got["kpt"] < 0, want["kpt"] < 0), label
    if c["metric"] == "pckh" or exact_terms:
        assert _same_bits(got["kpt"], want["kpt"]) and _same_bits(got["obj"], want["obj"]), label
    else:
        ratio_k = np.abs(got["kpt"] - want["kpt"]) / _term_bound(want["kpt"])
        ratio_o = np.abs(got["obj"] - want["obj"]) / lat.oks_budget(want["kpt"])
        print(f"{label}: worst ratio term {ratio_k.max(initial=0):.3f} object {ratio_o.max(initial=0):.3f}")
        assert (ratio_k <= 1).all() and (ratio_o <= 1).all(), label
    assert _same_bits(got["value"], want["value"]), label


@pytest.mark.parametrize("name", lat.LATTICE)
def test_lattice_is_separated(pkg, name):
    c, t, r = lat.case(name)
    assert lat.separation_violations(c, t, r) == 0
    assert (r["status"] == 0).all()


def test_lattice_covers_the_stated_shapes(pkg):
    seen_T, seen_P, seen_n, seen_K, seen_B = set(), set(), set(), set(), set()
    for name in lat.LATTICE:
        c, t, r = lat.case(name)
        tg = t["targets"]
        seen_K.add(c["K"])
        seen_B.add(len(c["images"]))
        seen_T |= set(np.diff(tg["t_off"]).tolist())
        seen_P |= {len(s) for _, s in t["preds"]}
        seen_n |= set((tg["t_xyv"][..., 2] > 0).sum(-1).tolist())
    assert {0, 1, 7, 8, 9, 128} <= seen_T and {1, 2, 30} <= seen_P and {1, 7, 8, 17} <= seen_n and {3, 17} <= seen_K and {1, 5} <= seen_B
    c, t, r = lat.case("k17_mixed")
    assert t["targets"]["t_area"][0] == 2.0 ** -52 and r["match"][0] == 2 and r["obj"][0] == 1.0  # no polygon; two exact hits, the first in the walk wins
    assert r["match"][6] == r["match"][7] == 5  # two targets take one prediction
    assert c["images"][3]["flag"] == 1 and r["value"][4] == -1.0
    c, t, r = lat.case("k3")
    assert r["match"][0] == 0  # equal scores: the lower index is first in the walk
    c, t, r = lat.case("pckh")
    assert r["obj"][1] == -1.0 and (r["kpt"][1] == -1.0).all() and set(np.unique(r["kpt"])) <= {-1.0, 0.0, 1.0}


@pytest.mark.parametrize("name", lat.LATTICE)
def test_restatement_equals_the_references_functions(pkg, golden, name):
    c, t, r = lat.case(name)
    g = {k.split("/", 1)[1]: golden[k] for k in golden.files if k.startswith(name + "/")}
    tg = t["targets"]
    # the fixture was made from these very inputs
    assert np.array_equal(g["t_off"], tg["t_off"]) and _same_bits(g["t_xyv"], tg["t_xyv"]) and _same_bits(g["t_area"], tg["t_area"])
    assert _same_bits(g["t_head"], tg["t_head"]) and _same_bits(g["variances"], c["variances"])
    assert _same_bits(g["p_xy"], np.concatenate([xy for xy, _ in t["preds"]])) and _same_bits(g["p_score"], np.concatenate([s for _, s in t["preds"]]))
    assert np.array_equal(g["match"], r["match"])
    if c["metric"] == "pckh":
        assert np.array_equal(g["obj"], r["obj"]) and np.array_equal(g["value"], r["value"])
        return
    ratio = np.abs(g["obj"] - r["obj"]) / lat.oks_budget(r["kpt"])
    vb = lat.value_budget(r["obj"], tg["t_off"])
    print(f"{name}: worst object ratio {ratio.max(initial=0):.3f}, worst value difference {np.abs(g['value'] - r['value']).max():.3g} of {vb.max():.3g}")
    assert (ratio <= 1).all()
    assert (np.abs(g["value"] - r["value"]) <= vb).all()
    assert np.array_equal(g["calculate_OKS"], g["value"])  # calculate_OKS is match + reorder + image_OKS


@pytest.mark.parametrize("form", ["decode", "f64"])
@pytest.mark.parametrize("name", lat.LATTICE)
def test_host_twin_equals_restatement(ps, name, form):
    c, t, r = lat.case(name)
    kw = dict(decode=t["decode"], inv_affine=t["inv_affine"]) if form == "decode" else dict(preds=t["preds"])
    got = ps.score_host(t["targets"], metric=c["metric"], variances=c["variances"], alpha=c["alpha"], **kw)
    check_against(c, t, r, got, exact_terms=False, label=f"{name}/{form}")


DEFECT_CASE = {  # planted defect -> (case, image whose result must change)
    "descending_walk": ("k17_mixed", 0), "ge": ("k17_mixed", 0), "no_mask": ("k17_mixed", 1), "area_no_spacing": ("k17_mixed", 0),
    "vars_no_2": ("k3", 0), "no_round": ("k17_mixed", 1), "f32_skipped": ("k17_mixed", 1), "f32_on_fallback": ("k17_mixed", 3),
}


@pytest.mark.parametrize("defect", ref.DEFECTS)
def test_planted_defect_fails_its_case(pkg, defect):
    name, b = DEFECT_CASE[defect]
    c, t, r = lat.case(name)
    bad = lat.restated(c, defect)
    a, e = t["targets"]["t_off"][b], t["targets"]["t_off"][b + 1]
    match_differs = not np.array_equal(bad["match"][a:e], r["match"][a:e])
    with np.errstate(invalid="ignore"):
        obj_differs = not (np.abs(bad["obj"][a:e] - r["obj"][a:e]) <= lat.oks_budget(r["kpt"][a:e])).all()
    value_differs = not abs(bad["value"][b] - r["value"][b]) <= lat.value_budget(r["obj"], t["targets"]["t_off"])[b]
    assert match_differs or obj_differs or value_differs, defect
    if defect in ("descending_walk", "ge"):
        assert match_differs
    if defect == "no_round":
        assert value_differs and not obj_differs


def test_defect_list_is_the_one_tested():
    assert set(DEFECT_CASE) == set(ref.DEFECTS)


def test_nan_coordinate_sets_the_status_bit(ps):
    c, t, r = lat.case("k17_mixed")
    joints = t["decode"][0].copy()
    joints[1, 3, 5, 0] = np.nan
    got = ps.score_host(t["targets"], decode=(joints,) + t["decode"][1:], inv_affine=t["inv_affine"], variances=c["variances"])
    off = t["targets"]["t_off"]
    assert got["status"].tolist() == [0, ps.NONFINITE, 0, 0, 0] and np.isnan(got["value"][1])
    assert np.isnan(got["obj"][off[1]:off[2]]).all() and np.isnan(got["kpt"][off[1]:off[2]]).all() and (got["match"][off[1]:off[2]] == -1).all()
    keep = np.r_[0:off[1], off[2]:off[-1]]
    assert np.array_equal(got["match"][keep], r["match"][keep]) and _same_bits(got["value"][[0, 2, 3, 4]], r["value"][[0, 2, 3, 4]])
    preds = [(xy.copy(), s.copy()) for xy, s in t["preds"]]
    preds[2][1][0] = np.inf  # a person score
    got = ps.score_host(t["targets"], preds=preds, variances=c["variances"])
    assert got["status"].tolist() == [0, 0, ps.NONFINITE, 0, 0] and np.isnan(got["value"][2])
    # no prediction at all against targets: its own bit, never a silent score
    preds[0] = (np.zeros((0, 17, 2)), np.zeros(0))
    got = ps.score_host(t["targets"], preds=preds, variances=c["variances"])
    assert got["status"][0] == ps.NO_PRED and np.isnan(got["value"][0]) and got["match"][0] == -1


def test_empty_batch_and_empty_images(ps):
    K = 17
    empty = ps.make_targets(np.zeros((0, K, 3)), t_off=[0])
    out = ps.score_host(empty, preds=[], variances=ps.OKS_VARIANCES)
    assert out["value"].shape == (0,) and out["obj"].shape == (0,)
    two = ps.make_targets(np.zeros((0, K, 3)), t_off=[0, 0, 0])
    out = ps.score_host(two, preds=[(np.zeros((0, K, 2)), np.zeros(0)), (np.ones((2, K, 2)), np.array([0.1, 0.2]))])
    assert out["value"].tolist() == [-1.0, -1.0] and out["status"].tolist() == [0, 0]


def _refused(ps, pkg, text, targets, **kw):
    with pytest.raises(pkg._lib.HHError, match=text):
        ps.score_host(targets, **kw)


def test_library_refusals(ps, pkg):
    c, t, r = lat.case("k3")
    tg, preds, var = t["targets"], t["preds"], c["variances"]
    _refused(ps, pkg, "image 0 has 129 targets, over HH_POSE_MAX_T", *lat.over_the_maxima("targets")[:1], preds=lat.over_the_maxima("targets")[1])
    _refused(ps, pkg, "image 0 has 65 predictions, over HH_POSE_MAX_P", *lat.over_the_maxima("predictions")[:1], preds=lat.over_the_maxima("predictions")[1])
    many = ps.make_targets(np.ones((1, 65, 3)))
    _refused(ps, pkg, "K outside 1..HH_POSE_MAX_K", many, preds=[(np.ones((1, 65, 2)), np.ones(1))], variances=np.ones(65))

    def edited(**changes):
        out = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in tg.items()}
        for k, (idx, val) in changes.items():
            out[k][idx] = val
        return out

    no_label = edited(t_xyv=((1, slice(None), 2), 0.0))
    _refused(ps, pkg, "image 0: target 1 has no labelled joint", no_label, preds=preds, variances=var)
    _refused(ps, pkg, "image 0: target 0 has a non-finite value", edited(t_xyv=((0, 1, 0), np.nan)), preds=preds, variances=var)
    for bad_area in (0.0, -1.0, np.inf, np.nan):
        _refused(ps, pkg, "image 0: target 1: area must be finite and > 0", edited(t_area=(1, bad_area)), preds=preds, variances=var)
    _refused(ps, pkg, "head size must be finite and >= 0", edited(t_head=(0, -1.0)), preds=preds, variances=var, metric="pckh")
    for bad_var in (0.0, np.inf, np.nan):
        _refused(ps, pkg, "vars must be finite and > 0", tg, preds=preds, variances=np.array([0.01, bad_var, 0.01]))
    _refused(ps, pkg, "t_off does not start at 0", dict(tg, t_off=np.array([1, 2], np.int32)), preds=preds, variances=var)
    two = dict(tg, t_off=np.array([0, 2, 1], np.int32))
    _refused(ps, pkg, "image 1: t_off decreases", two, preds=preds + preds, variances=var)
    _refused(ps, pkg, "alpha is not finite", tg, preds=preds, variances=var, alpha=np.nan)
    d = lat.case("k17_mixed")[1]
    inv = d["inv_affine"].copy()
    inv[2, 4] = np.inf
    _refused(ps, pkg, "image 2: non-finite inverse matrix", d["targets"], decode=d["decode"], inv_affine=inv)
    wide = (np.zeros((1, 65, 3, 4), np.float32), np.zeros((1, 65), np.float32), np.ones(1, np.int32), None)
    _refused(ps, pkg, "max_people outside 1..HH_POSE_MAX_P", tg, decode=wide, inv_affine=lat.IDENTITY[None], variances=var)
    # raw calls: a null table, a misaligned fp64 table, an unknown form
    lib = pkg._lib.load()
    p = t["preds"][0]
    po, out = np.array([0, len(p[1])], np.int32), ps._outputs_host(1, 2, 3)
    outs = [out[k].ctypes.data for k in ("value", "obj", "kpt", "match", "status")]
    shifted = np.zeros(2 * 3 * 3 * 8 + 8, np.uint8)[4:]  # 4 bytes off an 8-byte boundary

    def call(form=ps.PRED_F64, t_xyv=tg["t_xyv"].ctypes.data, obj=outs[1]):
        return lib.hh_pose_score_host(form, 0, 1, 3, None, 0, 0, 0, None, 0, None, None, 0, None, po.ctypes.data, p[0].ctypes.data, p[1].ctypes.data,
                                      tg["t_off"].ctypes.data, t_xyv, tg["t_area"].ctypes.data, tg["t_head"].ctypes.data, np.asarray(var).ctypes.data, 0.5,
                                      outs[0], obj, outs[2], outs[3], outs[4])
    assert call() == 0
    assert call(t_xyv=None) == 1 and b"null pointer" in lib.hh_last_error()
    assert call(obj=None) == 1 and b"null pointer" in lib.hh_last_error()
    assert call(form=7) == 1 and b"form is neither" in lib.hh_last_error()
    if shifted.ctypes.data % 8 == 4:
        shifted[:tg["t_xyv"].nbytes] = tg["t_xyv"].reshape(-1).view(np.uint8)
        assert call(t_xyv=shifted.ctypes.data) == 1 and b"not 8-byte aligned" in lib.hh_last_error()


def test_packer(ps):
    K = 3
    person = {"keypoints": [10, 20, 2, 30, 40, 1, 0, 0, 0], "segmentation": [[0, 0, 10, 0, 10, 10, 0, 10], [0, 0, 4, 0, 0, 4]]}
    unlabelled = {"keypoints": [0] * 9, "segmentation": {"counts": [1, 2], "size": [4, 4]}}  # not a target: its run-length mask is never looked at
    t = ps.pack_targets([[person, unlabelled], None, [unlabelled]])
    assert t["t_off"].tolist() == [0, 1, 1, 1] and t["K"] == K and t["t_area"].tolist() == [100.0 + 8.0 + 2.0 ** -52] and t["t_head"].tolist() == [0.0]
    assert t["t_xyv"].tolist() == [[[10, 20, 2], [30, 40, 1], [0, 0, 0]]]
    assert ps.pack_targets([[dict(person, segmentation=[])]])["t_area"].tolist() == [2.0 ** -52]
    with pytest.raises(ValueError, match=r"image 1: object 0: pose_score: a run-length \(iscrowd\) segmentation on a labelled object"):
        ps.pack_targets([None, [dict(person, segmentation={"counts": [3], "size": [2, 2]})]])
    with pytest.raises(ValueError, match="image 0 has 129 labelled objects, over HH_POSE_MAX_T"):
        ps.pack_targets([[person] * 129])
    with pytest.raises(ValueError, match="object 1 has 2 keypoints, expected 3"):
        ps.pack_targets([[person, {"keypoints": [1, 1, 1, 2, 2, 2], "segmentation": []}]])
    with pytest.raises(ValueError, match="pass num_kpts"):
        ps.pack_targets([None])
    assert ps.pack_targets([None], num_kpts=17)["t_xyv"].shape == (0, 17, 3)
    h = ps.pack_targets([[dict(person, head_xyxy=(0, 0, 3, 4)), person]], "pckh", head_boxes=[[(0, 0, 3, 4), (1, 1, 1, 1)]])
    assert h["t_head"].tolist() == [5.0, 0.0] and h["t_area"].tolist() == [2.0 ** -52] * 2
    assert ps.pack_targets([[dict(person, head_xyxy=(0, 0, 6, 8))]], "pckh")["t_head"].tolist() == [10.0]
    with pytest.raises(ValueError, match="metric must be one of"):
        ps.pack_targets([[person]], "iou")


def test_polygon_area(ps, pkg):
    assert ps.polygon_area([0, 0, 10, 0, 10, 10, 0, 10]) == 100.0
    assert ps.polygon_area([0, 10, 10, 10, 10, 0, 0, 0]) == 100.0            # the other orientation
    assert ps.polygon_area([0, 0, 4, 0, 0, 3]) == 6.0
    assert ps.polygon_area([0, 0, 3, 0, 0, 3]) == 4.5                         # a half-integer area
    assert ps.polygon_area([0.9, 0.9, 10.9, 0.2, 10.5, 10.99, 0.1, 10.7]) == 100.0   # truncated toward zero first
    assert ps.polygon_area([-0.9, -0.9, 10, 0, 10, 10, 0, 10]) == 100.0      # ... toward zero, not down
    assert ps.polygon_area([-5, -5, 5, -5, 5, 5, -5, 5]) == 100.0
    assert ps.polygon_area([0, 0, 2, 2, 2, 0, 0, 2]) == 0.0                  # a bow tie: the signed halves cancel
    assert ps.polygon_area([]) == 0.0 and ps.polygon_area([1, 2]) == 0.0 and ps.polygon_area([1, 2, 3, 4]) == 0.0
    big = 2.0 ** 30
    assert ps.polygon_area([-big, -big, big, -big, big, big, -big, big]) == 2.0 ** 62
    for bad in ([0, 0, np.nan, 0, 1, 1], [0, 0, 2.0 ** 31, 0, 1, 1]):
        with pytest.raises(pkg._lib.HHError, match="hh_polygon_area"):
            ps.polygon_area(bad)
    rs = np.random.RandomState(0)
    for _ in range(20):
        poly = rs.uniform(-300, 300, 2 * rs.randint(3, 12))
        assert ps.polygon_area(poly) == ref.polygon_area(poly)


def test_the_references_signatures(ps, pkg, golden):
    """match_preds_to_targets, object_OKS, image_OKS, object_PCKh, image_PCKh as the reference calls them, on the fixture's inputs."""
    kp_mod = importlib.import_module(PKG + ".keypoints")
    assert all(getattr(kp_mod, n) is getattr(ps, n) for n in ("match_preds_to_targets", "object_OKS", "image_OKS", "object_PCKh", "image_PCKh", "pack_targets"))
    c, t, r = lat.case("k17_mixed")
    off, g_match, g_obj, g_val = t["targets"]["t_off"], golden["k17_mixed/match"], golden["k17_mixed/obj"], golden["k17_mixed/value"]
    for b, im in enumerate(c["images"][:4]):
        xy, sc = t["preds"][b]
        xy = xy if im["flag"] else xy.astype(np.float32)
        kp = im["t_xyv"].astype(np.int64)
        m = ps.match_preds_to_targets(xy, sc, kp[..., :2], kp[..., 2])
        assert m == g_match[off[b]:off[b + 1]].tolist()
        obj = np.array([ps.object_OKS(xy[m[j]], kp[j, :, :2], kp[j, :, 2], im["polygons"][j]) for j in range(len(kp))])
        assert (np.abs(obj - g_obj[off[b]:off[b + 1]]) <= lat.oks_budget(r["kpt"][off[b]:off[b + 1]])).all()
        assert abs(ps.image_OKS(xy[m], kp[..., :2], kp[..., 2], im["polygons"]) - g_val[b]) <= lat.value_budget(r["obj"], off)[b]
    assert ps.object_OKS(np.zeros((17, 2)), np.zeros((17, 2)), np.zeros(17), []) == -1
    assert ps.image_OKS(np.zeros((1, 17, 2)), np.zeros((1, 17, 2)), np.zeros((1, 17)), [[]]) == -1
    assert ps.match_preds_to_targets(np.zeros((0, 17, 2)), np.zeros(0), np.ones((2, 17, 2)), np.ones((2, 17))) == [-1, -1]
    c, t, r = lat.case("pckh")
    off, g_match, g_obj, g_val = t["targets"]["t_off"], golden["pckh/match"], golden["pckh/obj"], golden["pckh/value"]
    for b, im in enumerate(c["images"]):
        xy, _ = t["preds"][b]
        kp = im["t_xyv"].astype(np.int64)
        m = g_match[off[b]:off[b + 1]].tolist()
        obj = [ps.object_PCKh(xy[m[j]], kp[j, :, :2], kp[j, :, 2], im["heads"][j], 0.5) for j in range(len(kp))]
        assert obj == g_obj[off[b]:off[b + 1]].tolist()
        assert ps.image_PCKh(0.5, xy[m], kp[..., :2], kp[..., 2], im["heads"]) == g_val[b]


def test_result_calculate_oks(ps, pkg, golden):
    """InferenceKeypointsResult.calculate_OKS on the fixture's images: the reference's assertion text without an annotation, -1 without a
    labelled object, otherwise the reference's value; nothing is reordered in place."""
    Result = importlib.import_module(PKG + ".keypoints.results").InferenceKeypointsResult
    c, t, r = lat.case("k17_mixed")
    off = t["targets"]["t_off"]

    def result(b, annot):
        xy, sc = t["preds"][b]
        im = c["images"][b]
        xy = xy if im["flag"] else xy.astype(np.float32)
        return Result(None, annot, None, xy, np.zeros(xy.shape[:2], np.float32), np.zeros(xy.shape[:2] + (1,), np.float32), sc.astype(xy.dtype), 0.05, 0.5)

    with pytest.raises(AssertionError, match="Matching preds to targets is possible only when annotation is set"):
        result(0, None).calculate_OKS()
    assert result(4, []).calculate_OKS() == -1
    assert result(4, [{"keypoints": [0] * 51, "segmentation": []}]).calculate_OKS() == -1
    for b in range(4):
        im = c["images"][b]
        annot = [{"keypoints": im["t_xyv"][j].astype(int).reshape(-1).tolist(), "segmentation": im["polygons"][j]} for j in range(len(im["t_xyv"]))]
        res = result(b, annot)
        before = res.kpts_coords.copy()
        assert res.oks is None and res.object_oks is None and res.kpt_oks is None and res.target_matches is None
        value = res.calculate_OKS()
        assert abs(value - golden["k17_mixed/calculate_OKS"][b]) <= lat.value_budget(r["obj"], off)[b]
        assert value == res.oks == res.calculate_OKS() and np.array_equal(res.kpts_coords, before)
        assert res.target_matches.tolist() == r["match"][off[b]:off[b + 1]].tolist() and res.kpt_oks.shape == (off[b + 1] - off[b], 17)


def test_blob_capacity_and_coco_variances(ps):
    """The device output block's size is a power of two from 4 KB up whatever the target count (so pinned result buffers keyed on it
    are a handful), and the layout inside does not depend on it; the COCO constants are refused for another number of keypoints."""
    sizes = {ps.DeviceScore.capacity(ps.DeviceScore.layout(32, T, 17)[1]) for T in range(0, 33)}
    assert sizes == {4096, 8192} and ps.DeviceScore.capacity(1) == 4096 and ps.DeviceScore.capacity(4097) == 8192
    lay, n = ps.DeviceScore.layout(2, 3, 17)
    raw = np.arange(ps.DeviceScore.capacity(n), dtype=np.uint8)
    parts = ps.DeviceScore(None, 2, 3, 17).split(raw)
    assert parts["kpt"].shape == (3, 17) and parts["status"].tobytes() == raw[n - 8:n].tobytes() and lay["value"][0] == 0
    assert ps.coco_variances(17) is ps.OKS_VARIANCES
    for K in (3, 16, 18):
        with pytest.raises(ValueError, match="17 COCO keypoints"):
            ps.coco_variances(K)
    with pytest.raises(ValueError, match="17 COCO keypoints"):
        ps.object_OKS(np.zeros((16, 2)), np.ones((16, 2)), np.ones(16), [])
    assert ps.object_PCKh(np.zeros((16, 2)), np.zeros((16, 2)), np.ones(16), (0, 0, 3, 4)) == 1.0
    stage = ps.TableStage()
    try:
        a = stage.take(100)
    except RuntimeError:  # (no accelerator runtime to page-lock with on this machine)
        return
    assert stage.take(4000) is a and a.numel() == 4096 and stage.take(5000).numel() == 8192


def test_fixture_is_small_and_described():
    meta = json.load(open(os.path.join(REPO, "tests", "golden", "pose_score_meta.json")))
    assert set(meta["cases"]) == set(lat.LATTICE) and "UNPINNED" in meta and os.path.getsize(GOLDEN) < 100 * 1024
    for name in lat.LATTICE:
        assert meta["cases"][name]["seed"] == lat.case(name)[0]["seed"]
