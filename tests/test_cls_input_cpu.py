"""Host half of the classifier's device-built input (classification/input.py), the reference / budget of tests/cls_input_budget.py
and the argument checks of hh_resized_crop_u8_batch: no GPU needed."""
import ctypes as C
import importlib

import numpy as np
import pytest
import torch

import cls_input_budget as cb
from conftest import PKG


@pytest.fixture(scope="module")
def ci_mod():
    return importlib.import_module(PKG + ".classification.input")


@pytest.fixture(scope="module")
def refs():
    """Per lattice case, computed once: (image, float64 restatement, budget, torch CPU)."""
    out = {}
    for c in cb.CASES:
        img = cb.image_of(c)
        ref = cb.restate(img, c)
        out[c.name] = (img, ref, cb.budget(c, ref), cb.torch_cpu(img, c).numpy())
    return out


@pytest.mark.parametrize("case", cb.CASES, ids=lambda c: c.name)
def test_budget_admits_torch_cpu(refs, case):
    """Not too tight: torch's own fp32 result lies within the derived budget of the float64 restatement, on EVERY element."""
    _, ref, allowed, got = refs[case.name]
    assert got.shape == (3, case.H, case.W) and np.isfinite(ref).all() and (allowed > 0).all()
    ratio = cb.worst_ratio(got, ref, allowed)
    print(f"{case.name}: torch CPU at {ratio:.4f} of the budget (largest allowance {allowed.max():.3e})")
    assert ratio <= 1.0, (case.name, ratio)


# (seeded mistake, the lattice cases it is planted in): each must exceed the budget by FACTOR on at least one of them.  The images
# are noise, so a tap moved by one pixel changes a [0,1] value by ~0.1 where the budget allows < 1e-3: three orders of magnitude;
# a factor of 100 leaves one of them to the luck of the draw.
FACTOR = 100.0
MISTAKES = [
    ("no_antialias", ["down-37x53", "window-120x47", "tall-500x40"]),       # antialias dropped on down-scaling cases
    ("clamp_image", ["corner-tl", "inner-crop", "down-8-crop"]),            # taps clamped to the image instead of the crop (they leave it at the bottom / right)
    ("flip_source", ["window-odd-flip", "window-120x47-flip"]),             # flip applied to the source crop, not the window
    ("origin_off_by_one", ["window-120x47", "window-odd-flip"]),            # window origin off by one
]


@pytest.mark.parametrize("mistake,names", MISTAKES, ids=[m for m, _ in MISTAKES])
def test_budget_flags_seeded_mistakes(refs, mistake, names):
    """Not too loose."""
    by_name = {c.name: c for c in cb.CASES}
    ratios = {}
    for name in names:
        img, ref, allowed, _ = refs[name]
        ratios[name] = cb.worst_ratio(cb.restate(img, by_name[name], mistake=mistake), ref, allowed)
    print(mistake, ratios)
    assert max(ratios.values()) >= FACTOR, (mistake, ratios)


def test_budget_flags_floor_in_the_centre_crop_offset(refs, ci_mod):
    """int(round(.)) replaced by floor in the CenterCrop offset: 40 x 70 -> Resize 32 -> CenterCrop 29 has offsets 1.5 and 13.5."""
    c = next(c for c in cb.CASES if c.name == "infer-40x70-29")
    assert (c.rh, c.rw, c.oy, c.ox) == ci_mod.inference_geometry(40, 70, 32, 29) == (32, 56, 2, 14)
    floored = c._replace(oy=(c.rh - 29) // 2, ox=(c.rw - 29) // 2)
    assert (floored.oy, floored.ox) == (1, 13)
    img, ref, allowed, _ = refs[c.name]
    ratio = cb.worst_ratio(cb.restate(img, floored), ref, allowed)
    print("floor_offset", ratio)
    assert ratio >= FACTOR


@pytest.mark.parametrize("name", cb.IDENTITY)
def test_identity_crops_are_bit_identical_to_torch(refs, name):
    """Extent == virtual size: every weight is exactly 1 or 0, so the restatement run in fp32 (division by 255, subtraction, division)
    equals torch bit for bit, and the float64 restatement rounds to within the normalise's two roundings of it."""
    c = next(c for c in cb.CASES if c.name == name)
    img, ref, allowed, got = refs[name]
    fp32 = cb.restate(img, c, dtype=np.float32)
    assert fp32.dtype == np.float32 and np.ascontiguousarray(fp32).tobytes() == np.ascontiguousarray(got).tobytes()
    # and it is the plain Normalize(ToTensor(.)) of the source pixels
    src = img[c.top:c.top + c.ch, c.left:c.left + c.cw].transpose(2, 0, 1)
    if c.flip:
        src = src[:, :, ::-1]
    plain = (src.astype(np.float32) / np.float32(255) - np.asarray(cb.MEAN, np.float32)[:, None, None]) / np.asarray(cb.STD, np.float32)[:, None, None]
    assert np.ascontiguousarray(plain).tobytes() == np.ascontiguousarray(got).tobytes()


def test_inference_geometry_hand_cases(ci_mod):
    g = ci_mod.inference_geometry
    assert g(40, 70, resize=32, crop=28) == (32, 56, 2, 14)
    assert g(70, 40, resize=32, crop=28) == (56, 32, 14, 2)          # portrait: the short side is the width
    assert g(40, 70, resize=32, crop=29) == (32, 56, 2, 14)          # odd differences 3 and 27: 1.5 -> 2, 13.5 -> 14 (floor: 1, 13)
    assert g(40, 70, resize=32, crop=27) == (32, 56, 2, 14)          # 5 and 29: 2.5 -> 2 (round half to even), 14.5 -> 14
    assert g(50, 50, resize=32, crop=28) == (32, 32, 2, 2)           # square
    assert g(375, 500) == (256, 341, 16, 58)                         # int(256 * 500 / 375) = 341; (341 - 224) / 2 = 58.5 -> 58
    assert g(300, 260) == (295, 256, 36, 16)
    # against F.interpolate to (rh, rw) followed by slicing, the definition itself
    rs = np.random.RandomState(3)
    for (h, w, resize, crop) in ((40, 70, 32, 28), (70, 40, 32, 29), (50, 50, 32, 28)):
        img = rs.randint(0, 256, (h, w, 3)).astype(np.uint8)
        rh, rw, oy, ox = g(h, w, resize, crop)
        assert min(rh, rw) == resize and 0 <= oy <= rh - crop and 0 <= ox <= rw - crop
        c = cb.Case("hand", h, w, 0, 0, h, w, rh, rw, oy, ox, crop, crop, 0, 1, 0)
        x = torch.from_numpy(img).permute(2, 0, 1).float().div(255)[None]
        full = torch.nn.functional.interpolate(x, size=(rh, rw), mode="bilinear", align_corners=False, antialias=True)[0]
        want = (full[:, oy:oy + crop, ox:ox + crop] - torch.tensor(cb.MEAN)[:, None, None]) / torch.tensor(cb.STD)[:, None, None]
        ref = cb.restate(img, c)
        assert cb.worst_ratio(want.numpy(), ref, cb.budget(c, ref)) <= 1.0


def test_random_resized_crop_params(ci_mod):
    draw = ci_mod.random_resized_crop_params
    torch.manual_seed(0)
    flips = 0
    for h, w in ((375, 500), (500, 375), (37, 53), (8, 8), (1, 1), (2000, 30)) * 20:
        p = draw(h, w)
        assert isinstance(p, ci_mod.CropParams) and all(isinstance(v, int) for v in (p.top, p.left, p.height, p.width))
        assert p.height > 0 and p.width > 0 and 0 <= p.top and p.top + p.height <= h and 0 <= p.left and p.left + p.width <= w, (h, w, p)
        flips += p.flip
    assert 30 < flips < 90  # 120 fair coins
    # equal seeds, equal draws (crop and flip)
    torch.manual_seed(5)
    a = [draw(375, 500) for _ in range(8)]
    torch.manual_seed(5)
    assert a == [draw(375, 500) for _ in range(8)] and len({(p.top, p.left, p.height, p.width) for p in a}) > 1
    # the fallback: in a 500 x 8 image (height x width) no size with a ratio in [3/4, 4/3] and >= 8 % of the area fits
    # (the width would have to be >= sqrt(0.08 * 4000 * 3/4) = 15.5), so all ten attempts fail: the central clamped-ratio crop
    torch.manual_seed(1)
    for _ in range(5):
        p = draw(500, 8)
        assert (p.top, p.left, p.height, p.width) == (244, 0, 11, 8)  # w = 8, h = round(8 / (3/4)) = 11, top = (500 - 11) // 2 = 244
    p = draw(8, 500)
    assert (p.top, p.left, p.height, p.width) == (0, 244, 8, 11)     # h = 8, w = round(8 * 4/3) = 11, left = (500 - 11) // 2 = 244
    assert ci_mod.central_crop_fallback(300, 300) == (0, 0, 300, 300)
    assert draw(10, 10, flip_p=None).flip is False


def test_descriptor_dtype_matches_the_struct(pkg, ci_mod):
    d = ci_mod._CROP_DESC
    assert d.itemsize == 56
    assert [d.fields[n][1] for n in d.names] == [0, 8, 12, 16, 20, 24, 28, 32, 36, 40, 44, 48, 52]
    assert d.names == ("image_offset", "h", "w", "top", "left", "ch", "cw", "rh", "rw", "oy", "ox", "flip", "antialias")
    header = open(pkg._lib.HEADER).read()
    body = header[header.index("typedef struct hh_crop_desc {"):header.index("} hh_crop_desc;")]
    assert [n for n in d.names if n not in body] == []
    offs, desc_off, target_off, total = ci_mod.ClsInput.layout([(37, 53), (13, 9)])
    assert list(offs) == [0, 5883, 6234] and desc_off == 6272 and target_off == 6272 + 112 and total == 6272 + 112 + 16


def _err(lib):
    return lib.hh_last_error().decode()


def test_refusals_before_any_device_call(pkg, ci_mod):
    """Every refusal returns on the host from the HOST copy of the descriptors: the non-null 'device' addresses are never
    dereferenced or passed on."""
    lib = pkg._lib.load()
    assert "hh_resized_crop_u8_batch" in pkg._lib.exported_symbols() and lib.hh_abi_version() == 3
    fake = 0x1000
    f3 = (C.c_float * 3)(0.5, 0.5, 0.5)
    good_desc = dict(image_offset=0, h=37, w=53, top=2, left=3, ch=20, cw=25, rh=16, rw=24, oy=0, ox=5, flip=0, antialias=1)

    def call(n=1, H=16, W=16, base=fake, ddev=fake, out=fake, mean=f3, std=f3, host=True, **over):
        descs = np.zeros(max(n, 1), ci_mod._CROP_DESC)
        for k, v in dict(good_desc, **over).items():
            descs[k] = v
        return lib.hh_resized_crop_u8_batch(base, ddev, descs.ctypes.data if host else None, n, out, H, W, mean, std, None)

    for kw in (dict(base=None), dict(ddev=None), dict(out=None), dict(mean=None), dict(std=None), dict(host=False)):
        assert call(**kw) != 0 and "null" in _err(lib), kw
    for kw in (dict(n=0), dict(n=70000), dict(H=0), dict(W=-3), dict(H=40000), dict(std=(C.c_float * 3)(0.5, 0.0, 0.5))):
        assert call(**kw) != 0 and "hh_resized_crop_u8_batch" in _err(lib), kw
    for kw, word in ((dict(ch=0), "extent"), (dict(cw=-1), "extent"), (dict(rh=0), "extent"), (dict(h=0), "extent"),
                     (dict(top=18), "outside its image"), (dict(left=29), "outside its image"), (dict(top=-1), "outside its image"),
                     (dict(left=2 ** 31 - 10), "outside its image"),
                     (dict(ox=9), "window outside"), (dict(oy=1), "window outside"), (dict(ox=-1), "window outside"), (dict(rw=15), "window outside"),
                     (dict(image_offset=-8), "offset"), (dict(h=30000, w=30000), "32-bit"), (dict(h=2 ** 24, w=1, top=0, ch=1, left=0, cw=1), "2^23")):
        assert call(**kw) != 0 and word in _err(lib) and "sample 0" in _err(lib), (kw, _err(lib))
    # the second sample is checked too
    descs = np.zeros(2, ci_mod._CROP_DESC)
    for k, v in good_desc.items():
        descs[k] = v
    descs[1]["ch"] = 36
    assert lib.hh_resized_crop_u8_batch(fake, fake, descs.ctypes.data, 2, fake, 16, 16, f3, f3, None) != 0 and "sample 1" in _err(lib)


def test_window_forms(ci_mod):
    ci = ci_mod.ClsInput(16, device="cpu")  # (no device work here)
    assert ci.resize == 18 and ci_mod.ClsInput(224, device="cpu").resize == 256
    w = ci.window(37, 53, ci_mod.CropParams(2, 3, 20, 25, True))
    assert (w.top, w.left, w.height, w.width, w.rh, w.rw, w.oy, w.ox, w.flip, w.antialias) == (2, 3, 20, 25, 16, 16, 0, 0, True, True)
    w = ci_mod.ClsInput(16, device="cpu", antialias=False).window(37, 53, (16, 24, 0, 5))
    assert (w.top, w.left, w.height, w.width, w.rh, w.rw, w.oy, w.ox, w.flip, w.antialias) == (0, 0, 37, 53, 16, 24, 0, 5, False, False)
    assert ci.window(1, 1, w) is w
