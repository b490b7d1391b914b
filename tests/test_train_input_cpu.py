"""Host half of the device-built training input (keypoints/train_input.py) and the argument checks of its C-ABI: no GPU needed.

The golden (tests/golden/train_input.npz, tools/make_train_input_golden.py) was produced by the reference's own
RandomAffineTransform / RandomHorizontalFlip / JointsGenerator / HeatmapGenerator / collate_fn on synth.synth_train_sample inputs;
only cv2.warpAffine was bound to oracle.transforms.warp_affine (cv2 parity UNPINNED, see the fixture's meta)."""
import ctypes as C
import shutil
import subprocess

import numpy as np
import pytest



from train_input_helpers import golden, golden_draw, golden_sample, golden_transform, ti_mod  # noqa: E402,F401


def test_golden_draws_matrices_and_joints(pkg, ti_mod, golden):
    """Equal seeds give the reference's augmentation: the same draws in the same order from the same global RNGs, matrices and
    float joints to rtol 1e-12 (float64 restatement; the same operation order in fact gives the same bits), integer joints and
    per-stage person lists exactly (the fixture keeps every transformed coordinate 1e-6 away from an integer)."""
    meta, data = golden
    assert {c["flip"] for c in meta["cases"]} == {True, False}
    for case in meta["cases"]:
        tag = case["tag"]
        _, _, joints = golden_sample(pkg, meta, case)
        ti, mode = golden_transform(ti_mod, meta, case)
        p, draws = golden_draw(mode, case)
        assert draws == case["draws"], tag
        assert p.flip == case["flip"], tag
        mat_image, mats, floats, ints = ti.geometry(case["h"], case["w"], joints, p)
        np.testing.assert_allclose(mat_image, data[f"{tag}.mat_image"], rtol=1e-12, atol=0, err_msg=tag)
        np.testing.assert_allclose(np.stack(mats), data[f"{tag}.mats"], rtol=1e-12, atol=0, err_msg=tag)
        for i in range(len(ti.hm_sizes)):
            np.testing.assert_allclose(floats[i], data[f"{tag}.joints_f{i}"], rtol=1e-12, atol=0, err_msg=tag)
            assert ints[i].dtype == np.int32 and np.array_equal(ints[i], data[f"{tag}.joints_i{i}"]), (tag, i)
            assert len(ints[i]) == case["people_per_stage"][i]


def test_mask_threshold_is_the_integer_test():
    """transforms.py:157-163: warpAffine(...) / 255 > 0.5 on a byte is v >= 128, for all 256 bytes."""
    v = np.arange(256, dtype=np.uint8)
    ref = ((v / 255) > 0.5).astype(np.float32)
    assert np.array_equal(ref, (v.astype(np.int32) >= 128).astype(np.float32))


@pytest.mark.parametrize("sigma", [1, 2, 4])
def test_bump_table_is_the_generators_bump_in_fp32(pkg, ti_mod, sigma):
    gen = pkg.keypoints.targets.HeatmapGenerator(17, 64 * sigma, sigma)
    table, reach = ti_mod.bump_table(sigma)
    assert table.dtype == np.float32 and table.flags.c_contiguous
    assert np.array_equal(table, gen.bump.astype(np.float32)) and reach == gen.reach == 3 * sigma + 1
    assert table.shape == (2 * reach + 1,) * 2 and table[reach, reach] == 1.0


def _err(lib):
    return lib.hh_last_error().decode()


def test_sigma_and_table_refusals(pkg, ti_mod):
    lib = pkg._lib.load()
    n, r = C.c_int(-1), C.c_int(-1)
    for sigma in (0.5, 1.5, 0.0, -1.0, float("nan"), float("inf")):  # 3 sigma + 1 not a positive integer
        assert lib.hh_heatmap_table_size(sigma, C.byref(n), C.byref(r)) != 0 and "hh_heatmap_table_size" in _err(lib), sigma
    assert lib.hh_heatmap_table_size(11.0, C.byref(n), C.byref(r)) != 0 and "63" in _err(lib)  # 6 * 11 + 3 = 69 entries
    assert (n.value, r.value) == (-1, -1)
    assert lib.hh_heatmap_table_size(2.0, None, C.byref(r)) != 0
    for sigma, want in ((1.0, (9, 4)), (2.0, (15, 7)), (4.0, (27, 13)), (10.0, (63, 31))):
        assert lib.hh_heatmap_table_size(sigma, C.byref(n), C.byref(r)) == 0 and (n.value, r.value) == want
    with pytest.raises(pkg._lib.HHError, match="3 \\* sigma \\+ 1"):
        ti_mod.bump_table(0.5)
    with pytest.raises(pkg._lib.HHError):  # sigma < 0 = size / 64 = 0.5 for a 32-pixel stage: refused before any GPU work
        ti_mod.TrainInput(128, [1 / 4, 1 / 2], sigma=-1)
    with pytest.raises(pkg._lib.HHError):
        ti_mod.TrainInput(128, [1 / 8] * 5)  # more stages than hh_train_desc holds


def test_null_and_range_refusals_before_any_device_call(pkg):
    """Every refusal below returns on the host: the non-null 'device' addresses are never dereferenced or passed on."""
    lib = pkg._lib.load()
    fake = 0x1000
    f3 = (C.c_float * 3)(0.5, 0.5, 0.5)
    # hh_render_heatmaps(joints, num_people, B, P, K, table, n, reach, out, h, w, stream)
    good = [fake, fake, 2, 3, 17, fake, 15, 7, fake, 32, 32, None]
    for idx in (0, 1, 5, 8):
        args = list(good)
        args[idx] = None
        assert lib.hh_render_heatmaps(*args) != 0 and "null" in _err(lib), idx
    for idx, bad in ((6, 0), (6, -1), (6, 65), (6, 13), (7, 6), (2, 0), (3, 0), (4, 0), (9, 0), (10, 0), (10, 4100), (2, 70000)):
        args = list(good)
        args[idx] = bad
        assert lib.hh_render_heatmaps(*args) != 0 and "hh_render_heatmaps" in _err(lib), (idx, bad)
    # hh_train_images_u8_batch(base, descs, n, out, H, W, mean, std, stream)
    good = [fake, fake, 2, fake, 128, 128, f3, f3, None]
    for idx in (0, 1, 3, 6, 7):
        args = list(good)
        args[idx] = None
        assert lib.hh_train_images_u8_batch(*args) != 0 and "null" in _err(lib), idx
    for idx, bad in ((2, 0), (2, 70000), (4, 0), (5, -3), (4, 1 << 24)):  # 2^24 x 128 pixels > 2^30
        args = list(good)
        args[idx] = bad
        assert lib.hh_train_images_u8_batch(*args) != 0 and "hh_train_images_u8_batch" in _err(lib), (idx, bad)
    # hh_train_masks_u8_batch(base, descs, n, nstages, stage_hw, out, stream)
    hw = (C.c_int * 10)(*[32] * 10)
    outs = (C.c_void_p * 5)(*[fake] * 5)
    good = [fake, fake, 2, 2, hw, outs, None]
    for idx in (0, 1, 4, 5):
        args = list(good)
        args[idx] = None
        assert lib.hh_train_masks_u8_batch(*args) != 0 and "null" in _err(lib), idx
    for nstages in (0, -1, 5):  # more stages than the struct holds
        assert lib.hh_train_masks_u8_batch(fake, fake, 2, nstages, hw, outs, None) != 0 and "stages" in _err(lib)
    assert lib.hh_train_masks_u8_batch(fake, fake, 0, 2, hw, outs, None) != 0
    assert lib.hh_train_masks_u8_batch(fake, fake, 2, 2, (C.c_int * 4)(32, 32, 0, 64), outs, None) != 0 and "positive" in _err(lib)
    assert lib.hh_train_masks_u8_batch(fake, fake, 2, 2, hw, (C.c_void_p * 2)(fake, None), None) != 0 and "null" in _err(lib)


def test_header_declares_exactly_what_the_library_exports(pkg):
    lib = pkg._lib.load()
    declared = set(pkg._lib.exported_symbols())
    nm = shutil.which("nm") or shutil.which("llvm-nm") or "/opt/rocm/llvm/bin/llvm-nm"
    out = subprocess.run([nm, "-D", "--defined-only", pkg._lib.SO], check=True, capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-1].startswith("hh_")}
    assert exported == declared, (sorted(exported - declared), sorted(declared - exported))
    new = {"hh_train_images_u8_batch", "hh_train_masks_u8_batch", "hh_heatmap_table_size", "hh_render_heatmaps"}
    assert new <= declared and lib.hh_abi_version() == 3
