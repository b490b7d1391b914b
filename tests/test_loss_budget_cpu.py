"""The references, budgets and lattices of tests/loss_budget.py, without a GPU: the op-by-op fp32 model of a correct kernel stays inside
every budget on every lattice case; every planted defect leaves a budget on a NAMED case (take that case out of the lattice and this
file fails); the lattice reaches the code paths it claims; the fp64 reference reproduces the reference-run goldens and agrees with the
independent restatement in oracle/loss.py; pack_joints' contract; the host-side refusals of the C-ABI."""
import importlib
import json
import os

import numpy as np
import pytest

import loss_budget as lb
from conftest import GOLDEN, PKG


@pytest.fixture(scope="module")
def lossmod():
    return importlib.import_module(PKG + ".keypoints.loss")


MSE = {lb.mse_name(c): c for c in lb.mse_cases()}


def _mse(prefix):
    """the case "BxKxhxw/mask/scale", whichever layout the lattice gives it"""
    (name,) = [n for n in MSE if n.rsplit("/", 1)[0] == prefix]
    return name, MSE[name]


# ---------------------------------------------------------------------------------------------------------------- model inside budget
def test_mse_model_stays_inside_every_budget():
    w = [0.0, 0.0]
    for name, case in MSE.items():
        (loss, grad), (a_loss, a_grad) = lb.mse_expected(case)
        got_loss, got_grad = lb.mse_fp32(*lb.mse_operands(case))
        r = lb.worst(got_loss, loss, a_loss), lb.worst(got_grad, grad, a_grad)
        assert all(v < 1 for v in r), (name, r)
        w = [max(a, b) for a, b in zip(w, r)]
        if case[1] == "zeros" or case[4]:  # an all-zero mask, pred == target: exact zeros
            assert got_loss == 0 and not got_grad.any() and loss == 0 and not grad.any(), name
    print(f"fp32 model of the MSE kernel: worst error / budget  loss {w[0]:.3f}  gradient {w[1]:.3f}")
    assert w[1] > 0.25  # the gradient budget is not slack: the model itself gets this close


def test_grouping_model_stays_inside_every_budget():
    w = {}
    for name, c in lb.grouping_cases().items():
        for ps, ls in lb.SCALES:
            ref = lb.grouping_expected(name, ps, ls)
            push, pull, grad = lb.grouping_model(c.tags, c.packed, c.counts, ps, ls)
            r = dict(push=lb.worst(push, ref.push, ref.allowed_push), pull=lb.worst(pull, ref.pull, ref.allowed_pull),
                     grad=lb.worst(grad, ref.grad, ref.allowed_grad))
            assert all(v < 1 for v in r.values()), (name, ps, ls, r)
            assert not grad[ref.hits == 0].any(), name
            for k, v in r.items():
                w[k] = max(w.get(k, 0.0), v)
    print("fp32 model of the grouping kernel: worst error / budget  " + "  ".join(f"{k} {v:.3f}" for k, v in w.items()))


def test_grouping_special_cases_are_exact_in_the_reference():
    z = lb.grouping_expected("nobody_visible", 0.25, 3.0)
    assert z.push == 0 and z.pull == 0 and not z.grad.any() and not z.hits.any()
    o = lb.grouping_expected("one_of_three_visible", 1.0, 0.0)
    assert o.push == 0 and not o.grad.any() and o.hits.sum() >= 3 and lb.grouping_expected("one_of_three_visible", 0.0, 1.0).grad.any()
    s = lb.grouping_expected("single_visible_joint", 0.0, 1.0)
    assert s.pull == 0 and not s.grad.any() and lb.grouping_expected("single_visible_joint", 1.0, 0.0).grad.any()
    a = lb.grouping_expected("tags_40_apart", 1.0, 0.0)
    assert a.push == 0 and not a.grad.any() and lb.grouping_expected("tags_40_apart", 0.0, 1.0).pull > 0
    i = lb.grouping_expected("identical_tags", 1.0, 1.0)
    assert i.push == 0.5 and i.pull == 0 and not i.grad.any()


def test_a_nan_or_inf_from_the_kernel_is_an_infinite_error():
    """`worst` never returns NaN (python's max and `<` would let one through): a non-finite result where the reference is finite is inf"""
    ref, allowed = np.array([1.0, 2.0]), np.array([1e-7, 1e-7])
    for bad in (np.nan, np.inf, -np.inf):
        assert lb.worst(np.array([1, bad], np.float32), ref, allowed) == np.inf
        assert lb.worst(np.array([bad, 2], np.float32), ref, allowed) == np.inf
        assert lb.worst(np.float32(bad), 1.0, 1e-7) == np.inf
        assert lb.worst(np.array([bad, 0], np.float32), np.zeros(2), np.zeros(2)) == np.inf  # also inside a zero budget
    assert lb.worst(np.array([1, 2], np.float32), ref, allowed) == 0.0 and lb.worst(np.zeros(2, np.float32), np.zeros(2), np.zeros(2)) == 0.0
    assert lb.worst(np.array([1, 2.5], np.float32), ref, np.array([1e-7, 0.0])) == np.inf  # a finite error outside a zero budget
    # and the model with NaN written into the gradient leaves the budget on a lattice case
    c = lb.grouping_cases()["K5_five_people"]
    ref = lb.grouping_expected(c.name, 1.0, 0.0)
    _, _, grad = lb.grouping_model(c.tags, c.packed, c.counts, 1.0, 0.0)
    grad[ref.hits > 0] = np.nan
    assert not lb.worst(grad, ref.grad, ref.allowed_grad) < 1


# ---------------------------------------------------------------------------------------------------------------- planted defects
MSE_FLAGGED_ON = {  # defect -> the case that must flag it, and the output that leaves its budget
    "mask_per_plane": ("2x17x8x8/binary/1", "grad"),
    "N_without_K": ("1x3x2x6/ones/1", "grad"),
    "no_factor_2": ("1x1x2x2/ones/1", "grad"),
    "tail_dropped": ("2x5x36x30/ones/1", "loss"),
    "planes_beyond_grid_dropped": ("61x17x4x4/ones/1", "loss"),
}
GROUPING_FLAGGED_ON = {
    "mean_over_K": ("K5_five_people", "pull"),
    "pull_over_listed": ("hole_between_two", "pull"),
    "push_n2": ("K5_five_people", "push"),
    "no_minus_n": ("tags_40_apart", "push"),
    "push_one_pair": ("K17_tall_map", "grad"),
    "xy_swapped": ("swap_safe_wide_map", "pull"),
    "overwrite_shared": ("two_on_one_pixel", "grad"),
    "no_div_B": ("K65", "push"),
    "read_padding": ("K64", "pull"),
}


def test_every_defect_has_a_named_case():
    assert set(MSE_FLAGGED_ON) == set(lb.MSE_DEFECTS) and set(GROUPING_FLAGGED_ON) == set(lb.GROUPING_DEFECTS)


@pytest.mark.parametrize("defect", lb.MSE_DEFECTS)
def test_planted_mse_defect_is_flagged(defect):
    prefix, output = MSE_FLAGGED_ON[defect]
    name, case = _mse(prefix)
    (loss, grad), (a_loss, a_grad) = lb.mse_expected(case)
    bad_loss, bad_grad = lb.mse_fp32(*lb.mse_operands(case), defect=defect)
    r = dict(loss=lb.worst(bad_loss, loss, a_loss), grad=lb.worst(bad_grad, grad, a_grad))
    print(f"{defect} on {name}: error / budget {r}")
    assert r[output] > 1, (defect, name, r)
    assert r["grad"] > 1  # (every MSE defect also shows in the gradient map)
    # the two loop defects show on no case that does not reach the loop
    if defect in ("tail_dropped", "planes_beyond_grid_dropped"):
        small = _mse("2x17x8x8/ones/1")[1]
        (l0, g0), (al0, ag0) = lb.mse_expected(small)
        bl, bg = lb.mse_fp32(*lb.mse_operands(small), defect=defect)
        assert lb.worst(bl, l0, al0) < 1 and lb.worst(bg, g0, ag0) < 1


@pytest.mark.parametrize("defect", lb.GROUPING_DEFECTS)
def test_planted_grouping_defect_is_flagged(defect):
    name, output = GROUPING_FLAGGED_ON[defect]
    c = lb.grouping_cases()[name]
    assert defect != "xy_swapped" or c.swap_safe
    r = {}
    for ps, ls in lb.SCALES:
        ref = lb.grouping_expected(name, ps, ls)
        push, pull, grad = lb.grouping_model(c.tags, c.packed, c.counts, ps, ls, defect=defect)
        r["push"] = lb.worst(push, ref.push, ref.allowed_push)
        r["pull"] = lb.worst(pull, ref.pull, ref.allowed_pull)
        r["grad"] = max(r.get("grad", 0.0), lb.worst(grad, ref.grad, ref.allowed_grad))
    print(f"{defect} on {name}: error / budget {r}")
    assert r[output] > 1, (defect, name, r)


# ---------------------------------------------------------------------------------------------------------------- coverage of the lattice
def test_the_lattice_reaches_what_it_claims():
    shapes = {c[0] for c in MSE.values()}
    planes = sorted(B * K for B, K, _, _ in shapes)
    groups = sorted(h * w // 4 for _, _, h, w in shapes)
    assert all(h * w % 4 == 0 for _, _, h, w in shapes)
    assert any(p > lb.PLANES_PER_LAUNCH for p in planes) and any(p > 2 * lb.PLANES_PER_LAUNCH for p in planes)  # two and three trips
    assert any(g > 256 and g % 256 for g in groups) and any(g < 256 for g in groups) and 1 in groups and any(g % 256 == 0 for g in groups)
    assert any(w % 4 for _, _, _, w in shapes)
    for shape in shapes:  # every shape meets every mask, scale and layout
        mine = [c for c in MSE.values() if c[0] == shape]
        assert {c[1] for c in mine} == set(lb.MSE_MASKS) and {c[2] for c in mine} == set(lb.MSE_SCALES)
        assert {c[3] for c in mine} == set(lb.MSE_LAYOUTS)
    assert any(c[4] for c in MSE.values())

    cases = lb.grouping_cases().values()
    assert {c.K for c in cases} >= {1, 5, 17, 64, 65, 130} and {(c.h, c.w) for c in cases} == {(4, 4), (6, 20), (20, 6), (32, 32)}
    assert {c.B for c in cases} >= {1, 3, 513} and any(2 * c.B > 1024 for c in cases)
    assert set(lb.grouping_cases()["ragged_0_to_33"].counts) == {0, 1, 2, 4, 5, 9, 33}
    assert set(lb.grouping_cases()["P257_P300"].counts) == {257, 300}
    assert any(c.P > 256 for c in cases) and {4, 5} <= {int(n) for c in cases for n in c.counts}
    assert any(c.sliced for c in cases)
    hit = {c.name: int(lb.grouping_expected(c.name, 1.0, 1.0).hits.max()) for c in cases}
    assert hit["two_on_one_pixel"] == 2 and hit["five_on_one_pixel"] == 5 and hit["P257_P300"] == 1
    for c in cases:
        live = np.concatenate([c.packed[b, :c.counts[b]].reshape(-1, 3) for b in range(c.B)])
        live = live[live[:, 2] > 0]
        assert ((live[:, 0] >= 0) & (live[:, 0] < c.w) & (live[:, 1] >= 0) & (live[:, 1] < c.h)).all(), c.name  # the C-ABI's contract
        pad = np.concatenate([c.packed[b, c.counts[b]:].reshape(-1, 3) for b in range(c.B)])
        assert ((pad[:, 0] >= 0) & (pad[:, 0] < c.w) & (pad[:, 1] >= 0) & (pad[:, 1] < c.h)).all(), c.name
        if c.name != "P257_P300":
            assert (pad[:, 2] > 0).all() and len(pad), c.name  # garbage a wrong kernel would count
        if c.swap_safe:
            assert c.h != c.w and (live[:, :2] < min(c.h, c.w)).all() and (live[:, 0] != live[:, 1]).all()
        if c.name == "four_corners":
            assert {(0, 0), (c.w - 1, 0), (0, c.h - 1), (c.w - 1, c.h - 1)} <= {(int(x), int(y)) for x, y, _ in live}
    wide = [c for c in cases if c.w > c.h]
    tall = [c for c in cases if c.h > c.w]
    assert any((c.packed[0, :c.counts[0], :, 0][c.packed[0, :c.counts[0], :, 2] > 0] >= c.h).any() for c in wide)
    assert any((c.packed[0, :c.counts[0], :, 1][c.packed[0, :c.counts[0], :, 2] > 0] >= c.w).any() for c in tall)
    vis = lb.grouping_cases()["K5_five_people"].packed[..., 2]
    assert {-1, 0, 1, 2} == set(np.unique(vis))


# ---------------------------------------------------------------------------------------------------------------- the reference itself
def test_reference_reproduces_the_goldens(pkg, lossmod):
    """tests/golden/loss.npz holds the reference project's own losses and autograd gradients; rtol 2e-5 and the atol of
    test_ae_loss_and_gradients_match_reference."""
    g = np.load(os.path.join(GOLDEN, "loss.npz"))
    meta = json.load(open(os.path.join(GOLDEN, "loss_meta.json")))
    for case in meta["cases"]:
        tag, B, size, people, seed, holes = case
        hms, masks, joints = pkg.synth.synth_train_targets(B, 17, size, people, seed=seed, mask_holes=holes)
        joints = pkg.synth.edit_loss_case(tag, joints)
        pred, tags = pkg.synth.synth_train_preds(hms, seed)
        mse = [lb.mse_reference(pred[i], hms[i], masks[i]) for i in range(2)]
        packed, counts = lossmod.pack_joints(joints[0], 17, size // 4, size // 4)
        gr = lb.grouping_reference(tags, packed, counts, 1e-3, 1e-3)
        losses = [mse[0][0], mse[1][0], 1e-3 * gr.push, 1e-3 * gr.pull]
        np.testing.assert_allclose(losses + [sum(losses)], g[f"{tag}.losses"], rtol=2e-5, atol=1e-9)
        flat = gr.grad.ravel()
        assert np.array_equal(np.flatnonzero(flat), g[f"{tag}.g_tags_idx"])
        np.testing.assert_allclose(flat[g[f"{tag}.g_tags_idx"]], g[f"{tag}.g_tags_val"], rtol=2e-5, atol=1e-10)
        for i in range(2):
            np.testing.assert_allclose(mse[i][1].ravel()[g[f"{tag}.g_pred{i}_idx"]], g[f"{tag}.g_pred{i}_val"], rtol=2e-5, atol=1e-10)


def test_reference_agrees_with_the_oracle_on_the_lattice():
    """oracle/loss.py states the same loss as python loops over people and joints (fp64 inside, results cast to fp32): an independent
    check of the vectorised reference, on every lattice case, to fp32 rounding plus the reference's own fp64 allowance."""
    from oracle import loss as ol
    for name, c in lb.grouping_cases().items():
        if c.B > 16:
            continue  # (the loops take seconds there; B enters both as one division)
        push, pull, gpush, gpull = ol.ae_grouping_loss(np.asarray(c.tags), lb.joints_lists(c))
        rp, rl = lb.grouping_expected(name, 1.0, 0.0), lb.grouping_expected(name, 0.0, 1.0)
        assert abs(push - rp.push) <= rp.allowed_push and abs(pull - rl.pull) <= rl.allowed_pull, name
        for got, ref in ((gpush, rp), (gpull, rl)):
            assert (np.abs(got - ref.grad) <= lb.U * np.abs(ref.grad) + ref.allowed_grad).all(), name
    for prefix in ("2x17x8x8/binary/1", "2x5x36x30/fractional/0.001"):
        name, case = _mse(prefix)
        p, t, m = lb.mse_operands(case)
        (loss, grad), (a_loss, a_grad) = lb.mse_expected(case)
        ol_loss, ol_grad = ol.heatmaps_loss(np.asarray(p), np.asarray(t), np.asarray(m))  # (fp32 op by op: a second model)
        assert abs(ol_loss - loss) <= a_loss and (np.abs(ol_grad - grad) <= a_grad).all(), name


# ---------------------------------------------------------------------------------------------------------------- the host side
def test_pack_joints_contract(lossmod):
    K, h, w = 3, 6, 20
    a = np.array([[[19, 5, 1], [-1, -6, 2], [0, 0, 0]], [[3, 2, 1], [25, 9, 0], [-30, 77, 0]]], np.int32)
    packed, counts = lossmod.pack_joints([a, np.zeros((0, K, 3), np.int32), a[:1]], K, h, w)
    assert packed.shape == (3, 2, K, 3) and packed.dtype == np.int32 and list(counts) == [2, 0, 1]
    assert packed[0, 0].tolist() == [[19, 5, 1], [19, 0, 1], [0, 0, 0]]  # negative coordinates wrap as tags[k, y, x] would
    assert packed[0, 1, :, 2].tolist() == [1, 0, 0]  # invisible joints outside the map pass
    assert not packed[1].any() and not packed[2, 1].any()  # the padding is zero
    for bad in ([20, 0, 1], [0, 6, 1], [-21, 0, 1], [0, -7, 2]):
        j = a.copy()
        j[1, 1] = bad
        with pytest.raises(IndexError):
            lossmod.pack_joints([j], K, h, w)
    j = a.copy()
    j[1, 1] = [20, 6, 0]
    lossmod.pack_joints([j], K, h, w)
    with pytest.raises(ValueError):
        lossmod.pack_joints([a], K + 1, h, w)


def test_device_joints_records_its_geometry(lossmod):
    import torch
    dj = lossmod.upload_joints([np.array([[[1, 2, 1]] * 3], np.int32)], 3, 8, 8, "cpu")
    assert dj.geometry == (3, 8, 8) and len(dj) == 1
    with pytest.raises(TypeError):
        lossmod.DeviceJoints(torch.zeros(1, 1, 3, 3, dtype=torch.int32), torch.zeros(1, dtype=torch.int32))


def test_c_abi_refusals_before_any_device_call(pkg):
    """Every refusal returns on the host: the non-null 'device' addresses are never dereferenced or passed on."""
    lib = pkg._lib.load()
    err = lambda: lib.hh_last_error().decode()  # noqa: E731
    A = 0x10000  # 16-byte aligned, never touched

    def mse(pred=A, bs=64, target=A, mask=A, B=1, K=1, h=8, w=8, loss=A, grad=A, gbs=64, scratch=A):
        return lib.hh_loss_heatmaps(pred, bs, target, mask, B, K, h, w, loss, grad, gbs, scratch, None)
    assert mse(h=3, w=3) != 0 and "multiples of 4" in err()
    assert mse(h=2, w=3) != 0 and mse(bs=66) != 0 and mse(gbs=66) != 0
    for arg in ("pred", "target", "mask", "grad"):
        for off in (4, 8, 12):
            assert mse(**{arg: A + off}) != 0 and "16-byte aligned" in err(), (arg, off)
    for arg in ("pred", "target", "mask", "loss", "scratch"):
        assert mse(**{arg: None}) != 0 and "bad argument" in err(), arg
    assert mse(B=0) != 0 and mse(K=0) != 0 and mse(h=0) != 0 and mse(w=-4) != 0

    def ae(tags=A, joints=A, counts=A, B=1, P=1, K=1, h=8, w=8, out=A, scratch=A):
        return lib.hh_loss_ae_grouping(tags, 64, joints, counts, B, P, K, h, w, out, A, 64, 1.0, 1.0, scratch, None)
    assert ae(P=2049) != 0 and "2048" in err()
    for arg in ("tags", "joints", "counts", "out", "scratch"):
        assert ae(**{arg: None}) != 0 and "bad argument" in err(), arg
    assert ae(B=0) != 0 and ae(P=0) != 0 and ae(K=0) != 0 and ae(h=0) != 0 and ae(w=0) != 0
