"""-m gpu: the classifier's input built on the device (hh_resized_crop_u8_batch, classification/input.py,
InferenceClassificationModel) against the float64 restatement and torch's fp32 CPU pipeline of tests/cls_input_budget.py, every element
within the derived budget; identity crops, repeats and single-sample launches bit for bit.

The output sizes are 16^2, 8^2 and the inference form's 28^2 / 29^2: the smallest at which each part can go wrong (several column
groups of a 32-wide tile are not needed for that: a tile column only ever sees its own taps; two tiles in height at 16, four at 28;
126 vertical taps over four LDS chunks at 500 x 40 -> 8^2).  One 224^2 inference sample covers a multi-tile output in both axes."""
import ctypes as C
import importlib

import numpy as np
import pytest
import torch

import cls_input_budget as cb
from conftest import PKG

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GROUPS = sorted({(c.H, c.W) for c in cb.CASES})


@pytest.fixture(scope="module")
def ci_mod():
    return importlib.import_module(PKG + ".classification.input")


@pytest.fixture(scope="module")
def refs():
    """Per lattice case, computed once and left unchanged: (image, float64 restatement, budget, torch CPU)."""
    out = {}
    for c in cb.CASES:
        img = cb.image_of(c)
        ref = cb.restate(img, c)
        out[c.name] = (img, ref, cb.budget(c, ref), cb.torch_cpu(img, c).numpy())
    return out


def pack(ci_mod, cases, images):
    """The images one after the other, each start moved on to the next offset that is NOT a multiple of 16 (so none is a multiple
    of 64), then the descriptors -> (host uint8 buffer, descriptor offset, descriptor view)."""
    offs, end = [], 0
    for im in images:
        offs.append(end + 1 if end % 16 == 0 else end)
        end = offs[-1] + im.size
    desc_off = (end + 7) // 8 * 8
    buf = np.zeros(desc_off + ci_mod._CROP_DESC.itemsize * len(cases), np.uint8)
    descs = buf[desc_off:].view(ci_mod._CROP_DESC)
    for b, (c, im) in enumerate(zip(cases, images)):
        buf[offs[b]:offs[b] + im.size] = im.reshape(-1)
        descs[b] = (offs[b], c.h, c.w, c.top, c.left, c.ch, c.cw, c.rh, c.rw, c.oy, c.ox, c.flip, c.aa)
    assert all(o % 64 for o in offs)
    return buf, desc_off, descs


def launch(pkg, ci_mod, cases, images, H, W, fill=float("nan"), expect_error=None):
    """hh_resized_crop_u8_batch through the C-ABI into a pre-filled buffer -> [n,3,H,W] numpy."""
    lib = pkg._lib.load()
    buf, desc_off, descs = pack(ci_mod, cases, images)
    raw = torch.from_numpy(buf).to(DEV)
    out = torch.full((len(cases), 3, H, W), fill, device=DEV, dtype=torch.float32)
    mean, std = (C.c_float * 3)(*cb.MEAN), (C.c_float * 3)(*cb.STD)
    rc = lib.hh_resized_crop_u8_batch(raw.data_ptr(), raw.data_ptr() + desc_off, descs.ctypes.data, len(cases), out.data_ptr(), H, W, mean, std,
                                      torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    if expect_error is None:
        pkg._lib.check(rc)
    else:
        assert rc != 0 and expect_error in lib.hh_last_error().decode(), lib.hh_last_error().decode()
    return out.cpu().numpy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def batches(pkg, ci_mod, refs):
    """Every lattice case, the cases of one output size as ONE batch of mixed raw sizes: {(H, W): (cases, [n,3,H,W])}."""
    out = {}
    for H, W in GROUPS:
        cases = [c for c in cb.CASES if (c.H, c.W) == (H, W)]
        out[(H, W)] = (cases, launch(pkg, ci_mod, cases, [refs[c.name][0] for c in cases], H, W))
    return out


@pytest.mark.parametrize("group", GROUPS, ids=lambda g: f"{g[0]}x{g[1]}")
def test_lattice_within_the_budget_of_float64_and_of_torch(batches, refs, group):
    """100 % of the elements within the derived budget of the float64 restatement AND of torch's fp32 CPU result; identity crops equal
    torch bit for bit.  (The buffer was pre-filled with NaN: an element that is not written fails.)"""
    cases, got = batches[group]
    assert len({(c.h, c.w) for c in cases}) > 1
    for b, c in enumerate(cases):
        _, ref, allowed, tcpu = refs[c.name]
        r64, r32 = cb.worst_ratio(got[b], ref, allowed), cb.worst_ratio(got[b], tcpu.astype(np.float64), allowed)
        print(f"{c.name}: at {r64:.4f} of the budget from float64, {r32:.4f} from torch CPU; identical to torch: {same_bits(got[b], tcpu)}")
        assert r64 <= 1.0 and r32 <= 1.0, (c.name, r64, r32)
        if c.name in cb.IDENTITY:
            assert same_bits(got[b], tcpu), c.name


def test_repeat_and_single_sample_launches_are_bit_identical(pkg, ci_mod, batches, refs):
    for group in ((16, 16), (8, 8)):
        cases, got = batches[group]
        images = [refs[c.name][0] for c in cases]
        assert same_bits(launch(pkg, ci_mod, cases, images, *group), got)
        for b in range(0, len(cases), 3):  # n = 1: the sample alone gives what it gives inside the batch
            assert same_bits(launch(pkg, ci_mod, [cases[b]], [images[b]], *group)[0], got[b]), cases[b].name


@pytest.mark.parametrize("crop", [28, 29])
def test_inference_form_through_build(ci_mod, refs, crop):
    """40 x 70 -> Resize 32 -> CenterCrop 28 / 29 (no multiple of anything): inference_geometry's parameters through ClsInput.build."""
    c = next(c for c in cb.CASES if c.name == f"infer-40x70-{crop}")
    img, ref, allowed, tcpu = refs[c.name]
    geometry = ci_mod.inference_geometry(40, 70, resize=32, crop=crop)
    assert geometry == (c.rh, c.rw, c.oy, c.ox)
    ci = ci_mod.ClsInput(crop, device=DEV)
    images, targets = ci.build([(img, 7), (img, 9)], [geometry, geometry])
    got = images.cpu().numpy()
    assert got.shape == (2, 3, crop, crop) and targets.dtype == torch.int64 and targets.tolist() == [7, 9] and targets.device == images.device
    assert same_bits(got[0], got[1])
    assert cb.worst_ratio(got[0], ref, allowed) <= 1.0 and cb.worst_ratio(got[0], tcpu.astype(np.float64), allowed) <= 1.0


def test_inference_at_224_against_torch_resize_and_slice(ci_mod):
    """ClsInput.inference at 224 on a 300 x 260 image (Resize 256 -> 295 x 256, CenterCrop 224 at (36, 16)): 28 x 7 tiles."""
    img = np.random.RandomState(21).randint(0, 256, (300, 260, 3)).astype(np.uint8)
    ci = ci_mod.ClsInput(224, device=DEV)
    assert ci.resize == 256
    images, targets = ci.inference([(img, 3)])
    c = cb.Case("infer-224", 300, 260, 0, 0, 300, 260, 295, 256, 36, 16, 224, 224, 0, 1, 0)
    ref = cb.restate(img, c)
    allowed, tcpu = cb.budget(c, ref), cb.torch_cpu(img, c).numpy()
    got = images.cpu().numpy()[0]
    r64, r32 = cb.worst_ratio(got, ref, allowed), cb.worst_ratio(got, tcpu.astype(np.float64), allowed)
    print(f"224^2 inference: at {r64:.4f} of the budget from float64, {r32:.4f} from torch CPU")
    assert r64 <= 1.0 and r32 <= 1.0 and targets.tolist() == [3] and (ci.last_launches, ci.last_h2d_bytes) == (1, ci.layout([(300, 260)])[3])


def test_refusals_leave_the_output_untouched(pkg, ci_mod, refs):
    """A rectangle outside the image, a window outside the virtual size, a zero extent: an error with a message before any launch;
    the output keeps its sentinel."""
    by_name = {c.name: c for c in cb.CASES}
    good = [by_name["corner-br"], by_name["window-120x47"]]
    images = [refs[c.name][0] for c in good]
    for cases, word in (([good[0]._replace(top=18), good[1]], "outside its image"), ([good[0], good[1]._replace(ox=9)], "window outside"),
                        ([good[0]._replace(cw=0), good[1]], "extent")):
        out = launch(pkg, ci_mod, cases, images, 16, 16, fill=7.0, expect_error=word)
        assert (out == 7.0).all(), word
    ci = ci_mod.ClsInput(16, device=DEV)
    with pytest.raises(pkg._lib.HHError, match="outside its image"):
        ci.build([(images[0], 0)], [ci_mod.CropParams(30, 0, 20, 25)])
    with pytest.raises(pkg._lib.HHError, match="window outside"):
        ci.build([(images[0], 0)], [(16, 24, 0, 9)])
    with pytest.raises(ValueError):
        ci.build([(images[0].astype(np.float32), 0)], [ci_mod.CropParams(0, 0, 20, 25)])
    got, _ = ci.build([(images[0], 0)], [ci_mod.CropParams(17, 28, 20, 25, True)])  # and goes on working
    assert same_bits(got.cpu().numpy()[0], launch(pkg, ci_mod, [good[0]], [images[0]], 16, 16)[0])


def test_train_batch_feeds_the_training_step(pkg, ci_mod):
    """ClsInput.train(samples) -> ClassificationModule.training_step for one step at B = 2: one launch, one copy of pixels +
    padding + descriptors + targets; shapes and dtypes accepted, the loss finite."""
    cls = importlib.import_module(PKG + ".classification")
    torch.manual_seed(0)
    model = cls.ClassificationModel(pkg.ClassificationHRNet(32, 1000))
    model.init_weights()
    model.to_CUDA(0)
    model.net.train()
    module = cls.ClassificationModule(model, cls.ClassificationLoss(), torch.optim.SGD(model.net.parameters(), lr=0.01))
    rs = np.random.RandomState(4)
    samples = [(rs.randint(0, 256, (75, 100, 3)).astype(np.uint8), 3), (rs.randint(0, 256, (90, 61, 3)).astype(np.uint8), 141)]
    ci = cls.ClsInput(64, device=DEV)
    torch.manual_seed(11)
    drawn = [cls.random_resized_crop_params(*s[0].shape[:2]) for s in samples]
    torch.manual_seed(11)
    images, targets = batch = ci.train(samples)  # the same draws from the same seed
    assert images.shape == (2, 3, 64, 64) and images.dtype == torch.float32 and images.is_cuda and images.is_contiguous()
    assert targets.dtype == torch.int64 and targets.tolist() == [3, 141] and bool(torch.isfinite(images).all())
    assert torch.equal(images, cls.ClsInput(64, device=DEV).build(samples, drawn)[0])
    pixels = sum(p.height * p.width * 3 for p in drawn)  # only the crops cross
    assert ci.last_launches == 1 and ci.last_h2d_bytes == (pixels + 63) // 64 * 64 + 2 * 56 + 2 * 8 < 75 * 100 * 3 + 90 * 61 * 3
    metrics = module.training_step(batch, 0)
    assert set(metrics) == {"loss", "top-1_error", "top-5_error"} and np.isfinite(metrics["loss"])
    # three builds in a row without a synchronisation (the third reuses the first's staging buffer) equal fresh builders' results
    params = [[cls.CropParams(k, 2 * k, 40, 50, bool(k % 2)), cls.CropParams(3, k, 60, 41 + k, False)] for k in range(3)]
    built = [ci.build(samples, p)[0] for p in params]
    torch.cuda.synchronize()
    for k in range(3):
        assert torch.equal(built[k], cls.ClsInput(64, device=DEV).build(samples, params[k])[0]), k
    assert not torch.equal(built[0], built[1])


def test_inference_model_batched_equals_single_calls(pkg):
    """InferenceClassificationModel on a seeded random-weight W32 net: infer_images of three images of different sizes equals three
    __call__s record for record; the prediction is the arg-max with the lower index on a tie; the probabilities sum to 1."""
    cls = importlib.import_module(PKG + ".classification")
    net = pkg.ClassificationHRNet(32, 1000)
    net.load_state_dict({k: torch.from_numpy(pkg.synth.synth_param(k, v.shape, 3)) for k, v in net.state_dict().items()})
    labels = {i: f"class-{i}" for i in range(1000)}
    model = cls.InferenceClassificationModel(net, labels, input_size=64, device=DEV)
    rs = np.random.RandomState(9)
    images = [rs.randint(0, 256, s + (3,)).astype(np.uint8) for s in ((80, 120), (150, 70), (64, 64))]
    x = model.prepare_input(images[0])
    assert x.shape == (1, 3, 64, 64) and x.dtype == torch.float32 and x.is_cuda
    batched = model.infer_images(images, target_labels=[5, "cat", None], max_batch=2)  # batches of 2 + 1
    assert len(batched) == 3
    for im, rb, t in zip(images, batched, [5, "cat", None]):
        r1 = model(im, t)
        assert rb.raw_image is im and rb.target_label == r1.target_label == t
        assert same_bits(rb.logits, r1.logits) and same_bits(rb.probs, r1.probs) and (rb.prediction, rb.pred_label) == (r1.prediction, r1.pred_label)
        assert rb.logits.shape == (1000,) and rb.logits.dtype == np.float32 and np.isfinite(rb.logits).all()
        assert rb.prediction == int(np.flatnonzero(rb.logits == rb.logits.max())[0]) and rb.pred_label == labels[rb.prediction]
        assert abs(float(rb.probs.sum(dtype=np.float64)) - 1.0) <= 1000 * 2.0 ** -24 and rb.probs.dtype == np.float32 and rb.probs.argmax() == rb.prediction
    assert len({r.logits.tobytes() for r in batched}) == 3
    # the tie rule on constructed logits: the lower index wins
    tie = torch.zeros(1, 1000)
    tie[0, 17] = tie[0, 400] = 2.5
    assert model._records([images[0]], tie, None)[0].prediction == 17
