"""Host half of the mosaic of the device-built training input (keypoints/train_input.py: Mosaic, mosaic_joints, mosaic_probability),
the resize restatement of tests/cv_resize.py and the argument checks of hh_mosaic_u8_batch: no GPU needed.

The golden (tests/golden/train_mosaic.npz, tools/make_train_mosaic_golden.py) was produced by the reference's own
CocoKeypointsDataset.__getitem__ / get_raw_mosaiced_data, transform and generators on a seeded pool; cv2.resize was bound to
tests/cv_resize.resize and cv2.warpAffine to oracle.transforms.warp_affine (cv2 parity UNPINNED, see the fixture's meta)."""
import random

import numpy as np
import pytest
import torch

import cv_resize as cv
from train_input_helpers import golden, golden_sample, golden_transform, ti_mod  # noqa: F401
from train_mosaic_helpers import MosaicRecorder, canvas_sha, golden_pool, mosaic_golden, pool_sha  # noqa: F401

S = 64
# the tile sizes of the GPU test at S = 64; AREA is the one that takes the 2 x 2 mean, IDENTITY the one that needs no resampling
SIZES = [(64, 64), (128, 128), (128, 100), (100, 128), (40, 56), (150, 97), (300, 260), (256, 256), (63, 65), (65, 63), (129, 127), (1, 1), (1, 200),
         (200, 1), (2, 2)]
AREA, IDENTITY = (128, 128), (64, 64)


def noise(h, w, seed=0):
    return np.random.RandomState(seed + 1000 * h + w).randint(0, 256, (h, w, 3)).astype(np.uint8)


# ------------------------------------------------------------------ the restatement
def test_identity_constant_and_area():
    img = noise(*IDENTITY)
    assert np.array_equal(cv.resize(img, (S, S)), img)                           # S x S comes back unchanged
    for h, w in SIZES:
        for v in (0, 1, 127, 200, 255):
            assert (cv.resize(np.full((h, w, 3), v, np.uint8), (S, S)) == v).all(), (h, w, v)   # a constant image stays constant
            assert (cv.resize(np.full((h, w), v, np.uint8), (S, S)) == v).all(), (h, w, v)
    img = noise(*AREA)
    mean = np.floor(img.astype(np.float64).reshape(S, 2, S, 2, 3).sum((1, 3)) / 4 + 0.5).astype(np.uint8)  # the rounded 2 x 2 mean
    assert np.array_equal(cv.resize(img, (S, S)), mean)
    # one axis at 2 alone stays bilinear: where 2 x 2 blocks exist (the leading S * 100 / 128 = 50 output columns resp. rows of a
    # 2S x 100 / 100 x 2S source) the result is NOT their mean, which a shortcut taken on one axis would give
    for h, w in ((128, 100), (100, 128)):
        img = noise(h, w)
        got = cv.resize(img, (S, S))
        blocks = cv.area_2x2(img.astype(np.int32)).astype(np.uint8)
        assert np.array_equal(got, cv.bilinear(img.astype(np.int32), S, S).astype(np.uint8))
        assert not np.array_equal(got[:blocks.shape[0], :blocks.shape[1]], blocks[:S, :S]), (h, w)
    # (at exactly 2 on both axes all four weights are 1024 and every shift of the two passes is exact: the bilinear formula gives
    # the 2 x 2 mean's bytes as well, so the shortcut OpenCV takes there cannot change a result)
    img = noise(*AREA, seed=5)
    assert np.array_equal(cv.bilinear(img.astype(np.int32), S, S), cv.area_2x2(img.astype(np.int32)))


def test_weights_sum_to_2048():
    for dst in (64, 96, 128, 512):
        for src in sorted({v for hw in SIZES for v in hw} | {480, 640, 1024, 427, 360, 3, 1000, 1333}):
            for column in (True, False):
                i0, i1, w0, w1 = cv.axis_taps(dst, src, column)
                assert ((w0 + w1) == cv.COEF_ONE).all() and w0.min() >= 0 and w1.min() >= 0, (dst, src, column)
                assert i0.min() >= 0 and i1.max() <= src - 1 and ((i1 - i0) >= 0).all() and ((i1 - i0) <= 1).all(), (dst, src, column)


def cross_check_budget(h, w):
    """Grey levels a byte of the fixed-point resize may lie from the exact bilinear value of the same pixel mapping, plus what
    torch's fp32 evaluation of that value may add.  From the quantisation steps:
      final          (t + 2) >> 2 rounds a sum of quarter grey levels to the nearest integer: 1/2;
      >> 16          each of the two products is truncated to quarter grey levels: 2 * 1/4;
      >> 4           each horizontal result (units of 1/2048) loses < 16/2048, combined with weights that sum to 1: 1/128;
      weights        a0 + a1 = 2048, so rounding them moves weight |d| <= 1/4096 between two bytes: 255 / 4096 per axis;
      coordinates    the restatement forms f in double and rounds once; torch forms scale, product and difference in fp32: together
                     <= 4 roundings of a value <= src, each src * 2^-24, times 255 per axis (the value is continuous in f);
      torch's sum    four products and three sums of values <= 255 in fp32: 8 * 255 * 2^-24."""
    return 0.5 + 2 * 0.25 + 1 / 128 + 2 * 255 / 4096 + 255 * 4 * (h + w) * 2.0 ** -24 + 8 * 255 * 2.0 ** -24


def test_cross_check_against_torch_bilinear():
    """Every byte of the non-area sizes against torch's float F.interpolate(bilinear, align_corners=False, antialias=False): guards the
    pixel mapping (tap positions, border handling, which axis is which); it is not cv2 parity."""
    worst, worst_budget = 0.0, 0.0
    for h, w in SIZES:
        if (h, w) == AREA:
            continue
        img = noise(h, w, seed=3)
        got = cv.resize(img, (S, S)).astype(np.float64)
        x = torch.from_numpy(img).permute(2, 0, 1)[None].float()
        ref = torch.nn.functional.interpolate(x, size=(S, S), mode="bilinear", align_corners=False, antialias=False)[0].permute(1, 2, 0).double().numpy()
        diff, budget = np.abs(got - ref).max(), cross_check_budget(h, w)
        print(f"resize cross-check {h}x{w} -> {S}: worst |diff| {diff:.4f} grey levels, budget {budget:.4f}")
        assert diff <= budget, (h, w, diff, budget)
        worst, worst_budget = max(worst, diff), max(worst_budget, budget)
    print(f"resize cross-check: worst {worst:.4f}, largest budget {worst_budget:.4f}")
    assert 1.0 < worst_budget < 1.25  # near one grey level: a misplaced tap on noise is tens of grey levels


# ------------------------------------------------------------------ joints
def test_mosaic_joints(pkg, ti_mod, mosaic_golden):
    meta, data = mosaic_golden
    for case in meta["cases"]:
        pool = golden_pool(pkg, meta, case)
        tiles = [pool[i] for i in case["tiles"]]
        got = ti_mod.mosaic_joints(tiles, meta["out_size"], meta["num_kpts"])
        want = cv.mosaic_reference(tiles, meta["out_size"])[2]
        assert got.dtype == np.float64 and got.shape == (case["people_on_canvas"], meta["num_kpts"], 3), case["tag"]
        assert np.array_equal(got, want) and np.array_equal(got, data[f"{case['tag']}.joints_canvas"]), case["tag"]
        assert pool_sha(pool) == case["pool_sha256"]  # the pool is not modified
        # tile order is kept and an empty tile contributes nothing
        counts = [len(t[2]) for t in tiles]
        assert sum(counts) == len(got)
        at = 0
        for i, (t, n) in enumerate(zip(tiles, counts)):
            one = ti_mod.mosaic_joints([t if j == i else (tiles[j][0], tiles[j][1], tiles[j][2][:0]) for j in range(4)], meta["out_size"], meta["num_kpts"])
            assert np.array_equal(one, got[at:at + n]), (case["tag"], i)
            at += n
        hidden = got[:, :, 2] <= 0
        assert hidden.any() and not got[hidden].any()  # invisible rows are zeroed
        vis = ~hidden
        if case["integer_joints"]:
            assert np.array_equal(got[vis], np.trunc(got[vis]))
        else:
            assert not np.array_equal(got[vis], np.trunc(got[vis]))
    assert {c["integer_joints"] for c in meta["cases"]} == {True, False}
    assert any(0 in [len(pool[i][2]) for i in c["tiles"]] and len(set(c["tiles"])) < 4 for c in meta["cases"])


def test_integer_joints_truncate_toward_zero(ti_mod):
    img, mask = np.zeros((30, 40, 3), np.uint8), np.ones((30, 40), bool)
    joints = np.zeros((1, 17, 3))
    joints[0, :, 0], joints[0, :, 1], joints[0, :, 2] = np.arange(17) - 8, 3 - np.arange(17), 1 + np.arange(17) % 2
    joints[0, 5, 2] = 0
    tiles = [(img, mask, joints)] + [(img, mask, joints[:0])] * 3
    as_float = ti_mod.mosaic_joints(tiles, 16)
    as_int = ti_mod.mosaic_joints([(img, mask, joints.astype(np.int32))] + tiles[1:], 16)
    want = joints.copy()
    want[0, :, 0], want[0, :, 1] = joints[0, :, 0] * (16 / 40), joints[0, :, 1] * (16 / 30)
    want[0, 5] = 0
    assert np.array_equal(as_float, want)
    assert np.array_equal(as_int[..., :2], np.trunc(want[..., :2])) and (np.trunc(want[0, :8, 0]) > want[0, :8, 0]).any()  # toward zero, not floor
    assert np.array_equal(joints[0, :, 0], np.arange(17) - 8)


# ------------------------------------------------------------------ draws
def test_probability_zero_draws_are_the_existing_goldens(pkg, ti_mod, golden):  # noqa: F811
    meta, _ = golden
    for case in meta["cases"]:
        ti, mode = golden_transform(ti_mod, meta, case, mosaic_probability=0.0)
        sample = golden_sample(pkg, meta, case)
        np.random.seed(case["rng_seed"])
        random.seed(case["rng_seed"])
        with MosaicRecorder() as rec:
            entries, params = mode.choose([sample], pool=None)
        assert rec.draws == case["draws"] and entries[0] is sample and params[0].flip == case["flip"], case["tag"]


def test_mosaic_draws_follow_the_reference(pkg, ti_mod, mosaic_golden):
    meta, _ = mosaic_golden
    S2 = 2 * meta["out_size"]
    for case in meta["cases"]:
        pool = golden_pool(pkg, meta, case)
        ti = ti_mod.TrainInput(meta["out_size"], meta["hm_resolutions"], num_kpts=meta["num_kpts"], sigma=meta["sigma"], **meta["transform"],
                               mosaic_probability=meta["mosaic_probability"])
        np.random.seed(case["rng_seed"])
        random.seed(case["rng_seed"])
        with MosaicRecorder() as rec:
            entries, params = ti.train.choose([pool[case["item"]]], pool)
        assert rec.draws == case["draws"], case["tag"]  # both global RNGs, in the reference's order
        assert [n for n, _ in rec.draws] == ["random.random"] + ["random.randint"] * 3 + ["np.random.random"] * 2 + ["np.random.randint"] * 2 + ["random.random"]
        assert isinstance(entries[0], ti_mod.Mosaic) and [t is pool[i] for t, i in zip(entries[0].tiles, case["tiles"])] == [True] * 4
        assert params[0].flip == case["flip"]
        # the AugParams are those of a 2S x 2S image
        np.random.seed(case["rng_seed"])
        random.seed(case["rng_seed"])
        random.random(), [random.randint(0, len(pool) - 1) for _ in range(3)]
        assert ti.train.draw(S2, S2) == params[0]
        assert pool_sha(pool) == case["pool_sha256"]


def test_non_mosaic_outcome_and_pool_requirement(pkg, ti_mod, mosaic_golden):
    meta, _ = mosaic_golden
    pool = golden_pool(pkg, meta, meta["cases"][0])
    ti = ti_mod.TrainInput(meta["out_size"], meta["hm_resolutions"], mosaic_probability=0.5)
    seed = next(s for s in range(100) if random.Random(s).random() >= 0.5)
    np.random.seed(seed)
    random.seed(seed)
    with MosaicRecorder() as rec:
        entries, params = ti.train.choose([pool[0]], pool)
    assert entries[0] is pool[0]
    assert [n for n, _ in rec.draws] == ["random.random"] + ["np.random.random"] * 2 + ["np.random.randint"] * 2 + ["random.random"]
    np.random.seed(seed)
    random.seed(seed)
    random.random()
    assert ti.train.draw(*pool[0][0].shape[:2]) == params[0]
    # inference honours the probability too (the dataset decides, not the transform): one draw, three tiles, then inference's two draws that change nothing
    seed = next(s for s in range(100) if random.Random(s).random() < 0.5)
    random.seed(seed)
    with MosaicRecorder() as rec:
        entries, params = ti.inference.choose([pool[0]], pool)
    assert isinstance(entries[0], ti_mod.Mosaic) and [n for n, _ in rec.draws] == ["random.random"] + ["random.randint"] * 3 + ["np.random.random"] * 2
    assert params[0] == ti_mod.AugParams(2 * meta["out_size"] / 200, 0.0, (float(meta["out_size"]), float(meta["out_size"])), False)
    for mode in (ti.train, ti.inference):
        with pytest.raises(ValueError, match="pool"):
            mode([pool[0]])
    with pytest.raises(ValueError):
        ti_mod.Mosaic(pool[:3])


# ------------------------------------------------------------------ golden canvases
def test_reference_reproduces_the_golden_canvases(pkg, mosaic_golden):
    meta, _ = mosaic_golden
    for case in meta["cases"]:
        pool = golden_pool(pkg, meta, case)
        canvas, canvas_mask, _ = cv.mosaic_reference([pool[i] for i in case["tiles"]], meta["out_size"])
        assert canvas.dtype == np.uint8 and canvas_mask.dtype == np.bool_ and canvas_sha(canvas, canvas_mask) == case["canvas_sha256"], case["tag"]


# ------------------------------------------------------------------ C-ABI
def _err(lib):
    return lib.hh_last_error().decode()


def test_refusals_before_any_device_call(pkg, ti_mod):
    """Every refusal returns on the host from the HOST copy of the descriptors: the non-null 'device' addresses are never
    dereferenced or passed on."""
    lib = pkg._lib.load()
    assert "hh_mosaic_u8_batch" in pkg._lib.exported_symbols() and lib.hh_abi_version() == 3
    fake = 0x1000

    def descs(n=1, tile=0, canvas_image_offset=4096, canvas_mask_offset=8192, **over):
        d = np.zeros(max(n, 1), ti_mod._MOSAIC_DESC)
        d["tile"]["h"], d["tile"]["w"] = 20, 30
        d["canvas_image_offset"], d["canvas_mask_offset"] = canvas_image_offset, canvas_mask_offset
        for k, v in over.items():
            d["tile"][k][-1, tile] = v  # the LAST sample: every sample is checked
        return d

    def call(n=1, S=64, base=fake, ddev=fake, host=True, **over):
        d = descs(n, **over)
        return lib.hh_mosaic_u8_batch(base, ddev, d.ctypes.data if host else None, n, S, None)

    for kw in (dict(base=None), dict(ddev=None), dict(host=False)):
        assert call(**kw) != 0 and "null" in _err(lib), kw
    for kw in (dict(n=0), dict(n=-1), dict(n=65536), dict(S=0), dict(S=2), dict(S=66), dict(S=-64), dict(S=8196), dict(base=fake + 2)):
        assert call(**kw) != 0 and "hh_mosaic_u8_batch" in _err(lib), kw
    for kw, word in ((dict(h=0), "extent"), (dict(w=-1), "extent"), (dict(h=30000, w=30000), "32-bit"), (dict(image_offset=-1), "negative offset"),
                     (dict(mask_offset=-8), "negative offset"), (dict(canvas_image_offset=-4), "negative canvas"),
                     (dict(canvas_mask_offset=-4), "negative canvas"), (dict(canvas_image_offset=4098), "multiples of 4"),
                     (dict(canvas_mask_offset=8193), "multiples of 4")):
        for n in (1, 3):
            for tile in (0, 3):
                assert call(n=n, tile=tile, **kw) != 0 and word in _err(lib) and f"sample {n - 1 if set(kw) & {'h', 'w', 'image_offset', 'mask_offset'} else 0}" in _err(lib), (kw, _err(lib))
                if set(kw) & {"h", "w", "image_offset", "mask_offset"}:
                    assert f"tile {tile}" in _err(lib)
    assert ti_mod._MOSAIC_DESC.itemsize == 112 and ti_mod._MOSAIC_DESC.fields["canvas_image_offset"][1] == 96
