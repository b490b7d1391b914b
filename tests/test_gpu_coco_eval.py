"""COCO keypoint scoring on the device (csrc/coco_eval.hip through hh_coco_oks / hh_coco_match / hh_coco_evaluate) against the host
evaluator on the lattice of tests/coco_eval_budget.py: OKS within the derived budget, everything downstream exactly equal."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

import coco_eval_budget as B
from conftest import PKG

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64  # bytes of 0xA5 in front of, between and behind the outputs


class DeviceTables:
    """One case's tables on the device (one copy) with the two hh_coco_tables structs."""

    def __init__(self, ce, t):
        blob, offs = ce.blob_layout(t)
        self.t, self.blob = t, torch.from_numpy(blob).to(DEV)
        self.dev = ce.tables_struct(t, lambda n: self.blob.data_ptr() + offs[n])
        self.host = ce.host_struct(t)
        self.A, self.T, self.N, self.M = len(t["area_rng"]), len(t["thr"]), len(t["dt_score"]), len(t["gt_area"])

    def args(self):
        return ctypes.byref(self.dev), ctypes.byref(self.host)


@pytest.fixture(scope="module")
def ce():
    return B.ce()


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg._lib.load()


@pytest.fixture(scope="module")
def tables(ce):
    return {name: DeviceTables(ce, B.case(name)[1]) for name in B.LATTICE}


def _stream():
    return torch.cuda.current_stream().cuda_stream


def run_matching(pkg, lib, dt, oks=None, shift=0):
    """hh_coco_evaluate (oks None) or hh_coco_match into outputs laid out in ONE 0xA5 buffer with guards; `shift` moves every output
    by that many ELEMENTS of its type.  Returns (dt_match, dt_ignore, gt_ignore, guard bytes)."""
    n, ng = dt.A * dt.T * dt.N, dt.A * dt.M
    at_m = GUARD + 4 * shift
    at_i = (at_m + 4 * n + GUARD + 3) // 4 * 4 + shift
    at_g = at_i + n + GUARD + shift
    total = at_g + ng + GUARD
    buf = torch.full((total,), 0xA5, dtype=torch.uint8, device=DEV)
    p = buf.data_ptr()
    if oks is None:
        rc = lib.hh_coco_evaluate(*dt.args(), p + at_m, p + at_i, p + at_g, _stream())
    else:
        rc = lib.hh_coco_match(*dt.args(), oks.data_ptr(), p + at_m, p + at_i, p + at_g, _stream())
    pkg._lib.check(rc)
    back = buf.cpu().numpy()
    dt_match = back[at_m:at_m + 4 * n].copy().view(np.int32).reshape(dt.A, dt.T, dt.N)
    dt_ignore, gt_ignore = back[at_i:at_i + n].reshape(dt.A, dt.T, dt.N), back[at_g:at_g + ng].reshape(dt.A, dt.M)
    guards = np.concatenate([back[:at_m], back[at_m + 4 * n:at_i], back[at_i + n:at_g], back[at_g + ng:]])
    return dt_match, dt_ignore, gt_ignore, guards


def _assert_equal_to_host(t, ref, got, oks_by_image=None):
    dtm, dti, gti = B.expected_tables(t, ref, oks_by_image)
    assert np.isin(got[1], (0, 1)).all() and np.isin(got[2], (0, 1)).all() and (got[0] >= 0).all() and (got[0] <= len(t["gt_area"])).all()  # all written
    assert np.array_equal(B.match_ids(t, got[0]), dtm) and np.array_equal(got[1] != 0, dti) and np.array_equal(got[2] != 0, gti)
    assert (got[3] == 0xA5).all()  # nothing around the three outputs was


@pytest.mark.parametrize("name", B.LATTICE)
def test_oks_within_budget(name, pkg, lib, tables):
    dt = tables[name]
    _, t, ref = B.case(name)
    n = int(t["oks_off"][-1])
    out = torch.full((n + 16,), float("nan"), dtype=torch.float64, device=DEV)
    pkg._lib.check(lib.hh_coco_oks(*dt.args(), out.data_ptr() + 8 * 8, _stream()))
    back = out.cpu().numpy()
    got, want, budget = back[8:8 + n], B.host_oks_flat(t, ref), B.budget_flat(t)
    err = np.where(np.isnan(got), np.inf, np.abs(got - want))
    print(f"{name}: {n} pairs, worst |error| / budget = {float((err / budget).max()):.3f}")
    assert (err <= budget).all()
    assert np.isnan(back[:8]).all() and np.isnan(back[8 + n:]).all()


@pytest.mark.parametrize("name", B.LATTICE)
def test_match_fed_the_host_matrix_is_exact(name, pkg, lib, tables):
    dt = tables[name]
    _, t, ref = B.case(name)
    oks = torch.from_numpy(np.concatenate([B.host_oks_flat(t, ref), [0.0]])).to(DEV)
    _assert_equal_to_host(t, ref, run_matching(pkg, lib, dt, oks))


@pytest.mark.parametrize("name", ["k17_special", "k17_words", "k1"])
def test_match_is_exact_on_adversarial_matrices(name, pkg, lib, tables):
    dt = tables[name]
    _, t, ref = B.case(name)
    for seed in (0, 1):
        by_image, flat = B.adversarial_oks(t, seed)
        _assert_equal_to_host(t, ref, run_matching(pkg, lib, dt, torch.from_numpy(flat).to(DEV)), by_image)


@pytest.mark.parametrize("name", B.LATTICE)
def test_fused_tables_and_stats_equal_the_host_evaluator(name, pkg, lib, tables, ce):
    dt = tables[name]
    c, t, ref = B.case(name)
    _assert_equal_to_host(t, ref, run_matching(pkg, lib, dt))
    ev = ce.COCOKeypointsEval(c["gts"], c["dets"], img_ids=ref["img_ids"], sigmas=c["sigmas"])
    stats = ev.evaluate(device=DEV)
    assert np.array_equal(ev.precision, ref["precision"]) and np.array_equal(ev.recall, ref["recall"]) and np.array_equal(stats, ref["stats"])
    assert ev.precision.shape == (10, 101, 3, 1) and ev.recall.shape == (10, 3, 1)


def test_nothing_is_carried_between_calls(pkg, lib, tables):
    a, b = tables["k17_words"], tables["k17_special"]
    first = run_matching(pkg, lib, a)
    again = run_matching(pkg, lib, a)
    other = run_matching(pkg, lib, b)
    third = run_matching(pkg, lib, a)
    for x in (again, third):
        assert all(np.array_equal(p, q) for p, q in zip(first, x))
    _assert_equal_to_host(b.t, B.case("k17_special")[2], other)


def test_odd_element_offset(pkg, lib, tables):
    _, t, ref = B.case("k17_words")
    _assert_equal_to_host(t, ref, run_matching(pkg, lib, tables["k17_words"], shift=1))
    _assert_equal_to_host(t, ref, run_matching(pkg, lib, tables["k17_words"], shift=3))


def test_two_launches_of_the_largest_case_give_equal_bytes(pkg, lib, tables):
    dt = tables[B.LARGEST]
    x, y = run_matching(pkg, lib, dt), run_matching(pkg, lib, dt)
    assert all(p.tobytes() == q.tobytes() for p, q in zip(x, y))
    n = int(dt.t["oks_off"][-1])
    o1, o2 = torch.zeros(n, dtype=torch.float64, device=DEV), torch.ones(n, dtype=torch.float64, device=DEV)
    pkg._lib.check(lib.hh_coco_oks(*dt.args(), o1.data_ptr(), _stream()))
    pkg._lib.check(lib.hh_coco_oks(*dt.args(), o2.data_ptr(), _stream()))
    assert torch.equal(o1, o2)


def test_over_the_limit_is_refused_on_the_device_too(pkg, lib, ce):
    dt = DeviceTables(ce, B.refusal_case())
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device=DEV)
    assert lib.hh_coco_evaluate(*dt.args(), buf.data_ptr(), buf.data_ptr() + (1 << 14), buf.data_ptr() + (1 << 15), _stream()) == 1
    assert "image 0 has 33 detections" in lib.hh_last_error().decode()
    assert int(buf.sum()) == 0


def test_evaluate_images_scores_its_packed_list(pkg, ce):
    """evaluate_images(..., gt_annotations=..., score_device=...): the packed list as before, plus the stats of that list by the device
    path, equal to scoring the list on the host."""
    ev_mod = importlib.import_module(PKG + ".keypoints.evaluation")
    net = pkg.HigherHRNet(17, 32)
    net.load_state_dict({k: torch.from_numpy(pkg.synth.synth_param(k, v.shape, 4)) for k, v in net.state_dict().items()})
    model = pkg.InferenceKeypointsModel(net.to(DEV).eval(), det_thr=0.05, tag_thr=0.5, use_flip=False, input_size=128, device=DEV)
    rs = np.random.RandomState(3)
    images = [rs.randint(0, 255, (100 + 20 * i, 160, 3)).astype(np.uint8) for i in range(4)]
    ids = [11, 12, 13, 14]
    plain = ev_mod.evaluate_images(model, images, ids)
    assert len(plain) >= 4
    # ground truths: the first two people found in every image, moved a little; one image without any
    gts = []
    for n, r in enumerate(plain):
        if r["image_id"] != 14 and sum(g["image_id"] == r["image_id"] for g in gts) < 2:
            k = np.asarray(r["keypoints"]).reshape(17, 3).copy()
            k[:, :2] += rs.normal(0, 1.5, (17, 2))
            k[:, 2] = 2
            gts.append(B.gt_person(r["image_id"], 500 + n, k, 60.0 ** 2))
    packed, stats = ev_mod.evaluate_images(model, images, ids, gt_annotations=gts, score_device=DEV)
    assert packed == plain
    host = ce.COCOKeypointsEval(gts, plain, img_ids=ids)
    assert np.array_equal(stats, host.evaluate()) and stats[0] > 0
