"""COCO keypoint scoring, the part that needs no GPU: csrc/coco_eval_math.h compiled for the host (hh_coco_evaluate_host) and the
vectorised pack / accumulate of keypoints/coco_eval.py against the host evaluator (COCOKeypointsEval._oks / _evaluate_img / evaluate)
on the lattice of tests/coco_eval_budget.py; the budget itself (neither too tight nor too loose); the refusals of the C-ABI."""
import ctypes
import importlib

import numpy as np
import pytest

import coco_eval_budget as B
from conftest import PKG

NEW_SYMBOLS = ("hh_coco_oks", "hh_coco_match", "hh_coco_evaluate", "hh_coco_evaluate_host")


@pytest.fixture(scope="module")
def ce():
    return B.ce()


def test_new_symbols_are_declared_and_exported(pkg):
    lib = pkg._lib.load()
    declared = pkg._lib.exported_symbols()
    for n in NEW_SYMBOLS:
        assert n in declared and hasattr(lib, n), n
    assert lib.hh_abi_version() == 3


@pytest.mark.parametrize("name", B.LATTICE)
def test_case_satisfies_the_separation_condition(name):
    c, t, ref = B.case(name)  # (raises if no seed does)
    assert B.separation_violations(t, ref) == 0 and len(t["img_ids"]) <= 12


def test_lattice_covers_the_counts(ce):
    Ds, Gs, Ks, raw_D = set(), set(), set(), set()
    for name in B.LATTICE:
        c, t, _ = B.case(name)
        Ds |= set(np.diff(t["dt_off"]).tolist())
        Gs |= set(np.diff(t["gt_off"]).tolist())
        Ks.add(c["K"])
        raw_D |= set(np.bincount([d["image_id"] for d in c["dets"]]).tolist())
    assert {0, 1, 3, 20} <= Ds and 25 in raw_D and max(Ds) == 20
    assert {0, 1, 2, 63, 64, 65, 128} <= Gs and Ks == {1, 17}
    t = B.case("k17_special")[1]
    edges = {np.nextafter(v, w) for v in (32.0 ** 2, 96.0 ** 2) for w in (0.0, v, np.inf)}
    assert edges <= set(t["gt_area"].tolist()) and edges <= set(t["dt_area"].tolist())
    assert {0.0, 1.0, 2.0} <= set(np.unique(B.case("k17_small")[1]["gt_xyv"][..., 2]).tolist())
    h = B.host_oks_flat(B.case("k17_areas")[1], B.case("k17_areas")[2])
    assert h.max() == 1.0 and h.min() < 1e-2


def test_special_situations_occur(ce):
    """The hand-placed images do what they were placed for, in the host evaluator's own results."""
    c, t, ref = B.case("k17_special")
    imgs = ref["imgs"][0]
    crowd_id = c["gts"][0]["id"]
    assert c["gts"][0]["iscrowd"] == 1 and (imgs[1]["dtMatches"][0] == crowd_id).sum() >= 3          # several detections on one crowd
    first, second = [g["id"] for g in c["gts"] if g["image_id"] == 2]
    oks = ref["oks"][2]
    assert oks[0, 0] == 1.0 and 0.8 < oks[0, 1] < 0.85
    assert imgs[2]["dtMatches"][0, 0] == second and imgs[2]["dtMatches"][-1, 0] == first            # the break rule decides below 0.83
    twin_a, _, twin_b = [g["id"] for g in c["gts"] if g["image_id"] == 3]
    assert ref["oks"][3][0, 0] == ref["oks"][3][0, 2] and imgs[3]["dtMatches"][0, 0] == twin_b and twin_a in imgs[3]["dtMatches"][0]
    o4 = ref["oks"][4]
    assert o4[0, 0] == 1.0 and o4[1, 0] == 1.0 and o4[2, 0] < 1.0 and o4[3, 0] == 1.0                # inside, edge, outside, between


@pytest.fixture(scope="module")
def host_form(ce):
    """hh_coco_evaluate_host on every case, once."""
    return {name: ce.match_tables_host(B.case(name)[1], want_oks=True) for name in B.LATTICE}


@pytest.mark.parametrize("name", B.LATTICE)
def test_host_form_oks_within_budget(name, host_form):
    _, t, ref = B.case(name)
    got, want, budget = host_form[name][3], B.host_oks_flat(t, ref), B.budget_flat(t)
    err = np.where(np.isnan(got), np.inf, np.abs(got - want))
    ratio = float((err / budget).max()) if err.size else 0.0
    print(f"{name}: {err.size} pairs, worst |error| / budget = {ratio:.3f}")
    assert err.size == t["oks_off"][-1] and (err <= budget).all()


@pytest.mark.parametrize("name", B.LATTICE)
def test_host_form_match_tables_equal_evaluate_img(name, host_form):
    _, t, ref = B.case(name)
    dtm, dti, gti = B.expected_tables(t, ref)
    got = host_form[name]
    assert np.array_equal(B.match_ids(t, got[0]), dtm) and np.array_equal(got[1], dti) and np.array_equal(got[2], gti)
    assert got[0].shape == (3, 10, len(t["dt_score"]))


@pytest.mark.parametrize("name", B.LATTICE)
def test_vectorised_accumulate_is_bit_identical(name, host_form, ce):
    _, t, ref = B.case(name)
    dt_match, dt_ignore, gt_ignore, _ = host_form[name]
    precision, recall = ce.accumulate_tables(t["dt_score"], dt_match, dt_ignore, gt_ignore)
    assert np.array_equal(precision, ref["precision"]) and np.array_equal(recall, ref["recall"])
    assert np.array_equal(ce.summarize(precision, recall), ref["stats"])
    assert (ref["stats"] > 0).any()


@pytest.mark.parametrize("name", ["k17_special", "k17_words", "k1"])
@pytest.mark.parametrize("seed", [0, 1])
def test_host_form_match_is_exact_on_adversarial_matrices(name, seed, ce):
    """Values exactly at a threshold, at 1 - 1e-10, at 1.0, all-equal rows: the separation condition is violated on purpose and the
    walk, fed the same matrix as _evaluate_img, must still agree exactly."""
    _, t, ref = B.case(name)
    by_image, flat = B.adversarial_oks(t, seed)
    dtm, dti, gti = B.expected_tables(t, ref, by_image)
    got = ce.match_tables_host(t, oks_in=flat)
    assert np.array_equal(B.match_ids(t, got[0]), dtm) and np.array_equal(got[1], dti) and np.array_equal(got[2], gti)
    assert (dtm != 0).any() and (dtm == 0).any()


def test_host_form_match_fed_the_evaluators_own_matrix(ce):
    for name in B.LATTICE:
        _, t, ref = B.case(name)
        got = ce.match_tables_host(t, oks_in=B.host_oks_flat(t, ref))
        dtm, dti, gti = B.expected_tables(t, ref)
        assert np.array_equal(B.match_ids(t, got[0]), dtm) and np.array_equal(got[1], dti) and np.array_equal(got[2], gti)


@pytest.mark.parametrize("name", B.LATTICE)
def test_budget_is_not_too_tight(name):
    """An honest fp64 implementation at the edge of what the budget allows for (the other summation order, every exp off by the two
    libraries' combined bound) stays inside on every pair."""
    _, t, ref = B.case(name)
    for i, img in enumerate(t["img_ids"]):
        want = np.asarray(ref["oks"][int(img)], np.float64)
        if want.size:
            assert (np.abs(B.oks_model(t, i, "nudged") - want) <= B.oks_budget(t, i)).all()


@pytest.mark.parametrize("defect", sorted(B.DEFECTS))
def test_budget_is_not_too_loose(defect):
    _, t, ref = B.case(B.DEFECTS[defect])
    outside = 0
    for i, img in enumerate(t["img_ids"]):
        want = np.asarray(ref["oks"][int(img)], np.float64)
        if want.size:
            outside += int((np.abs(B.oks_model(t, i, defect) - want) > B.oks_budget(t, i)).sum())
    assert outside > 0, f"{defect} stays inside the budget on {B.DEFECTS[defect]}"


@pytest.mark.parametrize("name", B.LATTICE)
def test_pack_tables_equals_the_evaluators_sort_and_cut(name, ce):
    c, t, ref = B.case(name)
    ev = ref["ev"]
    assert t["img_ids"].tolist() == ev.img_ids
    for i, img in enumerate(ev.img_ids):
        dts, gts = ev._dts[img], ev._gts[img]
        dts = [dts[j] for j in np.argsort([-d["score"] for d in dts], kind="mergesort")][: ce.MAX_DETS[-1]]
        d0, d1, g0, g1 = t["dt_off"][i], t["dt_off"][i + 1], t["gt_off"][i], t["gt_off"][i + 1]
        assert d1 - d0 == len(dts) and g1 - g0 == len(gts)
        assert t["dt_id"][d0:d1].tolist() == [d["id"] for d in dts] and t["gt_id"][g0:g1].tolist() == [g["id"] for g in gts]
        assert t["dt_score"][d0:d1].tolist() == [d["score"] for d in dts] and t["dt_area"][d0:d1].tolist() == [d["area"] for d in dts]
        assert t["dt_bbox"][d0:d1].tolist() == [list(map(float, d["bbox"])) for d in dts]
        K = c["K"]
        assert np.array_equal(t["dt_xy"][d0:d1], np.array([d["keypoints"] for d in dts], np.float64).reshape(len(dts), K, 3)[..., :2])
        assert t["gt_xyv"][g0:g1].reshape(len(gts), K * 3).tolist() == [g["keypoints"] for g in gts]
        assert t["gt_area"][g0:g1].tolist() == [g["area"] for g in gts] and t["gt_bbox"][g0:g1].tolist() == [g["bbox"] for g in gts]
        assert t["gt_flags"][g0:g1].tolist() == [int(g["ignore"]) + 2 * int(bool(g["iscrowd"])) for g in gts]
    assert np.array_equal(t["oks_off"], np.concatenate([[0], np.cumsum(np.diff(t["dt_off"]).astype(np.int64) * np.diff(t["gt_off"]))]))
    assert np.array_equal(t["vars"], (np.asarray(c["sigmas"]) * 2) ** 2)


def test_pack_tables_filters_images_and_categories(ce):
    c, _, _ = B.case("k17_small")
    other = [dict(c["dets"][0], category_id=2, score=2.0)]
    t = ce.pack_tables(c["gts"] + [dict(c["gts"][0], category_id=3)], c["dets"] + other, img_ids=[2, 3, 5])
    ev = ce.COCOKeypointsEval(c["gts"] + [dict(c["gts"][0], category_id=3)], c["dets"] + other, img_ids=[2, 3, 5])
    assert t["img_ids"].tolist() == [2, 3, 5]
    assert np.diff(t["dt_off"]).tolist() == [len(ev._dts[i]) for i in (2, 3, 5)] and np.diff(t["gt_off"]).tolist() == [len(ev._gts[i]) for i in (2, 3, 5)]
    default = ce.pack_tables(c["gts"], c["dets"])  # the evaluator's default: the images that have a result
    assert default["img_ids"].tolist() == ce.COCOKeypointsEval(c["gts"], c["dets"]).img_ids


def test_default_evaluate_is_the_host_evaluator(ce):
    """evaluate(device=None) is today's code path: the hand cases of the existing evaluator test, through the new signature."""
    ev_mod = importlib.import_module(PKG + ".keypoints.evaluation")
    rs = np.random.RandomState(0)
    gts, dets = [], []
    for img in (1, 2, 3):
        for p in range(2):
            k = np.concatenate([rs.uniform(50, 300, (17, 2)), np.full((17, 1), 2.0)], 1)
            gts.append(B.gt_person(img, 10 * img + p, k, 150.0 ** 2))
            dets += ev_mod.pack_coco_results(img, k[None, :, :2].astype(np.float32), np.array([0.9 - 0.1 * p], np.float32))
    ev = ce.COCOKeypointsEval(gts, dets)
    st = ev.evaluate(device=None)
    assert np.array_equal(st, ce.COCOKeypointsEval(gts, dets).evaluate())
    assert np.allclose(st[[0, 1, 2, 4, 5, 6, 7, 9]], 1.0) and st[3] == -1 and st[8] == -1
    fp = [dict(x, score=0.99, keypoints=(np.asarray(x["keypoints"]) + 1000).tolist()) for x in dets]
    st3 = ce.COCOKeypointsEval(gts, dets + fp).evaluate(None)
    assert abs(st3[0] - 0.5) < 0.02 and abs(st3[5] - 1.0) < 1e-9
    # and the vectorised path on the same hand cases, through the host form of the kernel
    t = ce.pack_tables(gts, dets + fp)
    p, r = ce.accumulate_tables(t["dt_score"], *ce.match_tables_host(t))
    assert np.array_equal(ce.summarize(p, r), st3)


# ------------------------------------------------------------------------------------------------ refusals
def _fake_device(ce, t):
    """hh_coco_tables of non-null, aligned addresses that point nowhere: a refused call must never look behind them."""
    return ce.tables_struct(t, lambda n: 0x7000000000 + 0x1000 * ce._TABLE_FIELDS.index(n))


def _all_entry_points(pkg, ce, t, host=None, tweak=None, out=(0x7100000000, 0x7100100000, 0x7100200000), null_host=False):
    """Call the four entry points on tables t (host struct optionally tweaked) and return their (rc, message) pairs."""
    lib = pkg._lib.load()
    host = host if host is not None else ce.host_struct(t)
    dev = _fake_device(ce, t)
    if tweak:
        tweak(host)
        tweak(dev)
    hp = None if null_host else ctypes.byref(host)
    res = []
    for call in (lambda: lib.hh_coco_oks(ctypes.byref(dev), hp, 0x7200000000, None),
                 lambda: lib.hh_coco_match(ctypes.byref(dev), hp, 0x7200000000, out[0], out[1], out[2], None),
                 lambda: lib.hh_coco_evaluate(ctypes.byref(dev), hp, out[0], out[1], out[2], None),
                 lambda: lib.hh_coco_evaluate_host(hp, None, None, out[0], out[1], out[2])):
        rc = call()
        res.append((rc, lib.hh_last_error().decode()))
    return res


def _refused(res, text, names=NEW_SYMBOLS):
    for (rc, msg), fn in zip(res, names):
        assert rc == 1 and msg.startswith(fn + ": ") and text in msg, (fn, rc, msg)


def test_refusals_return_1_before_anything_is_touched(pkg, ce):
    _, t, _ = B.case("k17_words")
    _refused(_all_entry_points(pkg, ce, t, null_host=True), "null pointer")
    for field in ("dt_off", "gt_off", "oks_off", "dt_xy", "dt_area", "gt_xyv", "gt_area", "gt_bbox", "gt_flags", "vars", "area_rng", "thr"):
        _refused(_all_entry_points(pkg, ce, t, tweak=lambda s, f=field: setattr(s, f, None)), "null pointer")
    for k in range(3):
        out = [0x7100000000, 0x7100100000, 0x7100200000]
        out[k] = None
        _refused(_all_entry_points(pkg, ce, t, out=tuple(out))[1:], "null pointer", NEW_SYMBOLS[1:])
    lib = pkg._lib.load()
    assert lib.hh_coco_oks(ctypes.byref(_fake_device(ce, t)), ctypes.byref(ce.host_struct(t)), None, None) == 1 and b"null pointer" in lib.hh_last_error()
    assert lib.hh_coco_evaluate(None, ctypes.byref(ce.host_struct(t)), 8, 8, 8, None) == 1 and b"null pointer" in lib.hh_last_error()

    def with_table(name, edit):
        arr = t[name].copy()
        edit(arr)
        return dict(t, **{name: arr})

    def set2(a, i, v):
        a[i] = v

    _refused(_all_entry_points(pkg, ce, with_table("dt_off", lambda a: set2(a, 2, a[1] - 1))), "non-monotone or out-of-range offsets at image 1")
    _refused(_all_entry_points(pkg, ce, with_table("gt_off", lambda a: set2(a, 1, a[2] + 1))), "non-monotone or out-of-range offsets at image 1")
    _refused(_all_entry_points(pkg, ce, with_table("dt_off", lambda a: set2(a, -1, a[-1] + 1))), "non-monotone or out-of-range offsets at image 5")
    _refused(_all_entry_points(pkg, ce, with_table("gt_off", lambda a: set2(a, -1, a[-1] - 1))), "offsets do not end at N and M")
    _refused(_all_entry_points(pkg, ce, with_table("dt_off", lambda a: set2(a, 0, 1))), "offsets do not start at 0")
    _refused(_all_entry_points(pkg, ce, with_table("gt_off", lambda a: set2(a, 1, 129))), "image 0 has 129 ground truths, over HH_COCO_MAX_GT (128)")
    _refused(_all_entry_points(pkg, ce, with_table("dt_off", lambda a: set2(a, 3, a[2] + 33))), "image 2 has 33 detections, over HH_COCO_MAX_DET (32)")
    _refused(_all_entry_points(pkg, ce, B.refusal_case()), "image 0 has 33 detections, over HH_COCO_MAX_DET (32)")
    _refused(_all_entry_points(pkg, ce, t, tweak=lambda s: setattr(s, "K", 65)), "K outside 1..64")
    _refused(_all_entry_points(pkg, ce, t, tweak=lambda s: setattr(s, "T", 17)), "T outside 1..HH_COCO_MAX_T (16)")
    _refused(_all_entry_points(pkg, ce, t, tweak=lambda s: setattr(s, "A", 5)), "A outside 1..HH_COCO_MAX_A (4)")
    _refused(_all_entry_points(pkg, ce, with_table("gt_area", lambda a: set2(a, 7, np.inf))), "non-finite ground-truth area")
    _refused(_all_entry_points(pkg, ce, with_table("dt_area", lambda a: set2(a, 7, np.nan))), "non-finite detection area")
    _refused(_all_entry_points(pkg, ce, with_table("vars", lambda a: set2(a, 3, 0.0))), "vars must be finite and > 0")
    _refused(_all_entry_points(pkg, ce, with_table("vars", lambda a: set2(a, 3, -1.0))), "vars must be finite and > 0")
    _refused(_all_entry_points(pkg, ce, with_table("vars", lambda a: set2(a, 16, np.inf))), "vars must be finite and > 0")
    _refused(_all_entry_points(pkg, ce, with_table("vars", lambda a: set2(a, 0, np.nan))), "vars must be finite and > 0")
