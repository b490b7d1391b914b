"""The segmentation overlay kernel and the dataset sample figures on the GPU (keypoints/sample_plot.py, hh_seg_overlay_u8_batch): the
device result is bit-identical to tests/seg_overlay_ref.py and to the host twin; the composed figures equal the composition of the numpy
references of each step."""
import io

import numpy as np
import pytest
import torch

import seg_overlay_ref as sr
from sample_plot_helpers import obj, overlay_cases, reference, rle_obj, sample_golden, sp  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _align(n, a=64):
    return (n + a - 1) // a * a


def _stage(sp, cases, poison: int):
    """One batch through the C ABI: [descriptors | shapes | toggles | frames at odd offsets | outputs at odd offsets] in one buffer filled
    with `poison`; every third frame is drawn in place.  -> (host bytes, descs, shapes, toggles, offsets, [(dst offset, size)])."""
    n = len(cases)
    num_shapes, num_toggles = sum(len(c[2]) for c in cases), sum(len(c[3]) for c in cases)
    shape_at = _align(sp.DESC.itemsize * n)
    toggle_at = _align(shape_at + 32 * num_shapes)
    at = _align(toggle_at + 4 * num_toggles)
    src_at, dst_at = [], []
    for j, c in enumerate(cases):
        size = c[1].size
        at = _align(at) + (1, 3, 2, 5)[j % 4]   # odd and even, never a multiple of 4 twice in a row
        src_at.append(at)
        at += size + 1
    for j, c in enumerate(cases):
        if j % 3 == 0:
            dst_at.append(src_at[j])
            continue
        at = _align(at) + (3, 1, 6, 7)[j % 4]
        dst_at.append(at)
        at += c[1].size + 1
    total = _align(at)
    host = np.full(total, poison, np.uint8)
    descs = host[:sp.DESC.itemsize * n].view(sp.DESC)
    shapes = host[shape_at:shape_at + 32 * num_shapes].view(np.int32).reshape(-1, 8)
    toggles = host[toggle_at:toggle_at + 4 * num_toggles].view(np.uint32)
    first = tog = 0
    for j, (_, image, s, t, alpha, bgr) in enumerate(cases):
        host[src_at[j]:src_at[j] + image.size] = image.reshape(-1)
        shapes[first:first + len(s)] = s
        shapes[first:first + len(s)][s[:, 0] == sr.FILL, 2] += tog
        toggles[tog:tog + len(t)] = t
        descs[j] = (src_at[j], dst_at[j], image.shape[0], image.shape[1], first, len(s), np.float32(1.0 - alpha), np.float32(alpha), 1 if bgr else 0, 0)
        first += len(s)
        tog += len(t)
    return host, descs, shapes, toggles, (shape_at, toggle_at), [(d, c[1].size) for d, c in zip(dst_at, cases)]


def _launch(pkg, sp, host, descs, shapes, toggles, offsets):
    buf = torch.from_numpy(host).to(DEV)
    base = buf.data_ptr()
    pkg._lib.launch(torch.device(DEV), pkg._lib.load().hh_seg_overlay_u8_batch, base, base, descs.ctypes.data, base + offsets[0], shapes.ctypes.data, len(shapes),
                    base + offsets[1], toggles.ctypes.data, len(toggles), len(descs))
    torch.cuda.synchronize()
    return buf.cpu().numpy()


@pytest.fixture(scope="module")
def batch(pkg, sp):
    cases = overlay_cases(sp)
    want = [reference(c) for c in cases]
    runs = []
    for poison in (0xA5, 0x5A, 0xA5):
        host, descs, shapes, toggles, offsets, dsts = _stage(sp, cases, poison)
        runs.append((host.copy(), _launch(pkg, sp, host, descs, shapes, toggles, offsets), dsts))
    return cases, want, runs


def test_device_equals_reference_and_host_twin(sp, batch):
    """One launch, mixed frames (1 x 1, 45 x 300, 64 x 37, around the tile size), odd source and destination offsets, in place and out of
    place, no shapes, clipping, draw order across chunks, a run-length fill, degenerate polygons, the B,G,R flag."""
    cases, want, runs = batch
    _, got, dsts = runs[0]
    assert any(d % 4 for d, _ in dsts) and any(d % 2 for d, _ in dsts)
    for case, ref, (at, size) in zip(cases, want, dsts):
        name, image, shapes, toggles, alpha, bgr = case
        out = got[at:at + size].reshape(image.shape)
        assert np.array_equal(out, ref), name
        assert np.array_equal(out, sp.overlay_host(image, shapes, toggles, alpha, bgr)), name


def test_only_dst_bytes_change_and_each_is_written(batch):
    """Nothing but the destination bytes changes in the staged buffer, and every destination byte is written: the result is the same
    over two different poison patterns, so no byte kept its poison."""
    cases, want, runs = batch
    for staged, got, dsts in runs:
        untouched = np.ones(staged.size, bool)
        for at, size in dsts:
            untouched[at:at + size] = False
        assert np.array_equal(got[untouched], staged[untouched])
    (_, a, dsts), (_, b, _), _ = runs
    for (at, size), ref in zip(dsts, want):
        assert np.array_equal(a[at:at + size], ref.reshape(-1)) and np.array_equal(b[at:at + size], ref.reshape(-1))


def test_same_bytes_on_every_run(batch):
    _, _, runs = batch
    assert np.array_equal(runs[0][1], runs[2][1])


def test_python_entry_points(pkg, sp):
    """overlay_frames_device with host and device frames in one call, in place and out of place; plot_segmentations."""
    cases = [c for c in overlay_cases(sp) if c[0] in ("crosses_tiles_45x300", "narrow_64x37", "rle", "no_shapes")]
    frames = [c[1] if j % 2 else torch.from_numpy(c[1]).to(DEV) for j, c in enumerate(cases)]
    outs = sp.overlay_frames_device(frames, [(c[2], c[3]) for c in cases], [c[4] for c in cases], [c[5] for c in cases])
    for c, f, o in zip(cases, frames, outs):
        assert np.array_equal(o.cpu().numpy(), reference(c)), c[0]
        if isinstance(f, torch.Tensor):
            assert np.array_equal(f.cpu().numpy(), c[1])  # the source is left as it was
    outs = sp.overlay_frames_device(frames, [(c[2], c[3]) for c in cases], [c[4] for c in cases], [c[5] for c in cases], in_place=True)
    for c, f, o in zip(cases, frames, outs):
        assert np.array_equal(o.cpu().numpy(), reference(c)), c[0]
        assert not isinstance(f, torch.Tensor) or o is f
    annot = [obj([5, 5, 60, 9, 30, 40]), obj([20, 2, 70, 30, 25, 44], [40, 20, 60, 20, 50, 35])]
    image = np.random.default_rng(3).integers(0, 256, (48, 80, 3), dtype=np.uint8)
    shapes, toggles = sp.seg_tables(annot, 48, 80)
    want = sr.overlay(image, shapes, toggles, np.float32(0.6), np.float32(0.4))
    assert np.array_equal(sp.plot_segmentations(image, annot), want)
    assert np.array_equal(pkg.keypoints.plot_segmentations(torch.from_numpy(image).to(DEV), annot, alpha=0.4), want)


# ---------------------------------------------------------------------------------------------------------------- the figures
def _ref_raw(sp, raw, annot, max_size):
    """plot_raw (coco.py:377-410) as the composition of the numpy references of its steps."""
    import cv_resize
    import render_ref as rr
    import text_ref
    h, w = raw.shape[:2]
    joints = sp.annot_joints(annot)
    img = rr.render(raw, joints[..., :2], joints[..., 2], sp.COCO_LIMBS, 0.5, "person", 0.8, sp.DEFAULT_PALETTE)
    shapes, toggles = sp.seg_tables(annot, h, w)
    img = sr.overlay(img, shapes, toggles, np.float32(1.0 - 0.4), np.float32(0.4))
    new_h, new_w, top, left = sp.letterbox(h, w, max_size)
    if (new_h, new_w) != (h, w):
        img = cv_resize.resize(img, (new_w, new_h))
    pane = np.zeros((max_size, max_size, 3), np.uint8)
    pane[top:top + new_h, left:left + new_w] = img
    return text_ref.put_txt(pane, ["Raw Image", f"Shape: {h} x {w}"])


def _ref_sample(sp, item, nrows=3, stage_idxs=(1,)):
    """plot (coco.py:412-449), line by line, on the numpy references."""
    import cv_resize
    import panels_ref as pr
    import render_ref as rr
    import text_ref
    raw, annot, (img, heatmaps, masks, joints_list), stem = item
    img_npy = pr.inverse_transform(img)
    lut = pr.jet_lut()
    grids = []
    for idx in stage_idxs:
        h, w = masks[idx].shape
        font_scale, labels = (0.5, ["Transformed Image", f"Sample: {stem}", f"Stage: {idx} ({h} x {w})"]) if idx == 1 else (0.25, [f"Stage: {idx} ({h} x {w})"])
        image = cv_resize.resize(img_npy, (w, h))
        cells = [pr.cell(image, hm, 0, lut) for hm in heatmaps[idx]]
        joints = np.asarray(joints_list[idx], np.float64)
        image = rr.render(image, joints[..., :2], joints[..., 2], sp.COCO_LIMBS, 0.5, "person", 0.8, sp.DEFAULT_PALETTE)
        mask = np.repeat((masks[idx] * 255).astype(np.uint8)[:, :, None], 3, 2)
        if idx == 1:
            cells = [text_ref.put_txt(c, [sp.COCO_LABELS[i]], alpha=0.8, font_scale=font_scale) for i, c in enumerate(cells)]
            mask = text_ref.put_txt(mask, ["Crowd Mask"], alpha=1, font_scale=font_scale)
        image = text_ref.put_txt(image, labels, alpha=0.8, font_scale=font_scale)
        grids.append(pr.make_grid([image, mask, *cells], nrows))
    mh, mw = max(g.shape[0] for g in grids), max(g.shape[1] for g in grids)
    model = pr.make_grid([g if g.shape[:2] == (mh, mw) else cv_resize.resize(g, (mw, mh)) for g in grids], len(grids))
    return pr.stack_horizontally([_ref_raw(sp, raw, annot, model.shape[0]), model])


def test_plot_raw_equals_the_composed_references(sp):
    from sample_plot_helpers import golden_items
    for raw, annot, _, _ in golden_items():
        for max_size in (163, 232, 90):
            assert np.array_equal(sp.plot_raw(raw, annot, max_size), _ref_raw(sp, raw, annot, max_size)), (raw.shape, max_size)
    raw, annot, _, _ = golden_items()[0]
    assert np.array_equal(sp.plot_raw_device(torch.from_numpy(raw).to(DEV), annot, 140).cpu().numpy(), _ref_raw(sp, raw, annot, 140))  # no resize at all


def test_plot_sample_equals_the_composed_references(sp, sample_golden):
    from sample_plot_helpers import golden_items
    meta, _ = sample_golden
    items = golden_items()
    for case in meta["samples"]:
        raw, annot, sample, stem = items[case["idx"]]
        kw = dict(nrows=case["kwargs"].get("nrows", 3), stage_idxs=tuple(case["kwargs"].get("stage_idxs", (1,))))
        got = sp.plot_sample(raw, annot, sample, stem, **kw)
        assert list(got.shape[:2]) == case["size"]
        assert np.array_equal(got, _ref_sample(sp, items[case["idx"]], **kw)), case["tag"]
    # device tensors in place of the arrays give the same figure
    raw, annot, (img, hms, masks, joints), stem = items[1]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    got = sp.plot_sample_device(t(raw), annot, (t(img), [t(h) for h in hms], [t(m) for m in masks], joints), stem, nrows=1, stage_idxs=(1, 0))
    assert np.array_equal(got.cpu().numpy(), _ref_sample(sp, items[1], 1, (1, 0)))


def test_plot_examples_and_jpeg_round_trip(sp, sample_golden):
    from PIL import Image
    from sample_plot_helpers import golden_items
    meta, _ = sample_golden
    items = [(raw, annot, sample, stem) for raw, annot, sample, stem in golden_items()]
    fig = sp.plot_examples(items)
    assert list(fig.shape[:2]) == meta["examples"]["size"] and fig.dtype == np.uint8
    plots = [_ref_sample(sp, it, 1, (1, 0)) for it in items]
    for p, (y, x, h, w) in zip(plots, meta["examples"]["grid"]["places"]):
        assert np.array_equal(fig[y:y + h, x:x + w], p)
    outside = np.ones(fig.shape[:2], bool)
    for y, x, h, w in meta["examples"]["grid"]["places"]:
        outside[y:y + h, x:x + w] = False
    assert not fig[outside].any()
    data = sp.plot_examples_jpeg(items)
    decoded = Image.open(io.BytesIO(data))
    assert decoded.size == (fig.shape[1], fig.shape[0]) and decoded.mode == "RGB"
    err = np.abs(np.asarray(decoded, np.int16) - fig.astype(np.int16))
    print(f"JPEG round trip of the figure: mean abs error {err.mean():.2f}, max {err.max()}")


def test_train_input_plot_examples(pkg, sp, sample_golden):
    """A dense-mask sample and a CrowdSegments / JpegImage sample in one call: a figure of the planned size; the batch that `build`
    returns is bit-identical with and without the plotting call."""
    from sample_plot_helpers import golden_items
    kp = pkg.keypoints
    meta, _ = sample_golden
    (raw0, annot0, _, _), (raw1, annot1, _, _) = golden_items()
    dense = np.ones(raw0.shape[:2], bool)
    dense[10:40, 20:70] = False
    jpeg_image = kp.JpegImage(kp.jpeg.encode_jpeg_host(raw1, quality=95, subsampling="444"))
    annotated = [(raw0, annot0, dense), (jpeg_image, annot1)]
    params = [kp.train_input.AugParams(90 / 200 * 1.1, 12.0, (72.0, 43.0), True), kp.train_input.AugParams(80 / 200 * 0.9, -7.0, (41.0, 63.0), False)]

    def batch(ti):
        samples = [(raw0, dense, kp.raw_sample(raw0, annot0)[2]), (jpeg_image, kp.CrowdSegments.from_annotations(annot1, 120, 80), kp.raw_sample(raw1, annot1)[2])]
        images, heatmaps, masks, joints = ti.build(samples, params)
        torch.cuda.synchronize()
        return [images.cpu()] + [t.cpu() for t in heatmaps + masks] + [j.packed.cpu() for j in joints] + [j.counts.cpu() for j in joints]

    fresh = batch(kp.TrainInput(128, [1 / 4, 1 / 2], device=DEV))
    ti = kp.TrainInput(128, [1 / 4, 1 / 2], device=DEV)
    before = batch(ti)
    fig = ti.plot_examples(annotated, params, names=["000000000139", "000000000785"])
    assert list(fig.shape[:2]) == meta["examples"]["size"] and fig.dtype == np.uint8 and fig.any()
    after = batch(ti)
    for a, b, c in zip(before, after, fresh):
        assert torch.equal(a, b) and torch.equal(a, c)
    # drawn params, the device form
    import random
    random.seed(3), np.random.seed(3)
    dev_fig = ti.plot_examples(annotated[1:], device_out=True)
    assert dev_fig.is_cuda and tuple(dev_fig.shape) == (20 + 173 + 20, 20 + 1504 + 20, 3)
    # a trainer configured with mosaic: the samples are plotted as plain samples, the augmentation drawn per sample
    mosaic_ti = kp.TrainInput(128, [1 / 4, 1 / 2], device=DEV, mosaic_probability=0.5)
    random.seed(4), np.random.seed(4)
    fig = mosaic_ti.plot_examples(annotated)
    assert list(fig.shape[:2]) == meta["examples"]["size"] and fig.any()
