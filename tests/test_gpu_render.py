"""-m gpu: the pose overlay kernel (hh_render_poses_u8_batch) and the general 8-bit resize (hh_resize_u8) against their numpy
restatements (tests/render_ref.py, tests/cv_resize.py), bit-identical on every byte, and the Python interface built on them
(plot_connections, InferenceKeypointsResult.plot, infer_images(render=...), video_frame).  Frame sizes and primitive counts are aimed
at the kernel's tile and chunk (hh_render_config)."""
import importlib

import numpy as np
import pytest
import torch

import cv_resize
import render_ref as rr
from conftest import PKG
from render_helpers import case_inputs, frame, lattice, reference, render_golden, vis  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FIELDS = ("kpts_coords", "kpts_scores", "kpts_tags", "obj_scores")


def _render(vis, frames, tables, alphas, bgr=False):
    return [vis.to_host(t) for t in vis.render_frames_device(frames, tables, alphas, bgr)]


@pytest.fixture(scope="module")
def cases(vis):
    """The lattice with its references, computed once."""
    return [(name, img, table, alpha, bgr, reference(img, table, alpha, bgr)) for name, img, table, alpha, bgr in lattice(vis, vis.render_config())]


def test_lattice_single_launches(vis, cases):
    for name, img, table, alpha, bgr, ref in cases:
        got = _render(vis, [img], [table], alpha, bgr)[0]
        assert got.shape == ref.shape and np.array_equal(got, ref), (name, int((got != ref).sum()))


def test_lattice_from_device_frames_at_odd_addresses(vis, cases):
    """Frames that are already on the device, at byte offsets 0..3 of an allocation: dword and byte paths of loads and stores."""
    for k, (name, img, table, alpha, bgr, ref) in enumerate(cases[::3]):
        buf = torch.zeros(img.size + 8, dtype=torch.uint8, device=DEV)
        view = buf[k % 4:k % 4 + img.size].view(img.shape)
        view.copy_(torch.from_numpy(img))
        got = vis.to_host(vis.render_frames_device([view], [table], alpha, bgr)[0])
        assert np.array_equal(got, ref), name
        assert np.array_equal(view.cpu().numpy(), img), name  # the source is only read


def test_batch_of_mixed_sizes_equals_single_launches(vis, cases):
    C = vis.render_config()[2]
    pick = [c for c in cases if c[0].startswith("mixed_") and c[0].endswith(("a0.8", "a0.65"))][::3] + [c for c in cases if c[0] == f"stack_{C + 1}"] + \
        [c for c in cases if c[0].startswith("empty_")][-1:]
    assert len(pick) >= 3 and len({c[1].shape for c in pick}) >= 3
    got = _render(vis, [c[1] for c in pick], [c[2] for c in pick], [c[3] for c in pick], [c[4] for c in pick])
    for g, c in zip(got, pick):
        assert np.array_equal(g, c[5]), c[0]
        assert np.array_equal(g, _render(vis, [c[1]], [c[2]], c[3], c[4])[0]), c[0]


def test_golden_through_plot_connections(pkg, vis, render_golden):
    meta, data = render_golden
    for c in meta["cases"]:
        img, coords, scores = case_inputs(data, c)
        before = img.copy()
        got = pkg.keypoints.plot_connections(img, coords, scores, meta["limbs"], c["thr"], c["color_mode"], c["alpha"])
        assert got.dtype == np.uint8 and np.array_equal(got, data[c["tag"] + ".out"]), c["tag"]
        assert np.array_equal(img, before)
    # the BGR flag on a golden case
    c = meta["cases"][1]
    img, coords, scores = case_inputs(data, c)
    table = vis.build_primitives(coords, scores, meta["limbs"], c["thr"], c["color_mode"], vis.DEFAULT_PALETTE, c["alpha"])
    assert np.array_equal(_render(vis, [img], [table], c["alpha"], True)[0], data[c["tag"] + ".out"][..., ::-1])


def test_golden_through_result_plot(pkg, render_golden):
    meta, data = render_golden
    c = next(c for c in meta["cases"] if c["tag"] == "person_a08")
    img, coords, scores = case_inputs(data, c)
    res = pkg.InferenceKeypointsResult(img, None, None, coords, scores, np.zeros(scores.shape + (1,)), np.ones(len(coords)), c["thr"], 0.5, meta["limbs"])
    plots = res.plot()
    assert set(plots) == {"connections"} and np.array_equal(plots["connections"], data["person_a08.out"])
    c = next(c for c in meta["cases"] if c["tag"] == "limb_a065")
    img, coords, scores = case_inputs(data, c)
    res = pkg.InferenceKeypointsResult(img, None, None, coords, scores, np.zeros(scores.shape + (1,)), np.ones(len(coords)), c["thr"], 0.5, meta["limbs"])
    assert np.array_equal(res.plot_connections("limb", 0.65), data["limb_a065.out"])


@pytest.fixture(scope="module")
def model(pkg):
    net = pkg.HigherHRNet(17, 32)
    net.load_state_dict({k: torch.from_numpy(pkg.synth.synth_param(k, v.shape, 3)) for k, v in net.state_dict().items()})
    return pkg.InferenceKeypointsModel(net.to(DEV).eval(), det_thr=0.05, tag_thr=0.5, use_flip=False, input_size=128, device=DEV)


def _expected_frame(res, color_mode, alpha, order=None):
    coords, scores = res.kpts_coords, res.kpts_scores
    if order is not None:
        coords, scores = coords[order], scores[order]
    palette = importlib.import_module(PKG + ".keypoints.visualization").DEFAULT_PALETTE
    return rr.render(res.raw_image, coords, scores, res.limbs, res.det_thr, color_mode, alpha, palette)


def test_infer_images_render(model):
    rs = np.random.RandomState(9)
    images = [rs.randint(0, 255, s + (3,)).astype(np.uint8) for s in [(150, 220), (220, 150), (150, 220), (128, 128), (150, 221)]]
    plain = model.infer_images(images, max_batch=2)
    drawn = model.infer_images(images, max_batch=2, render=dict(color_mode="limb", alpha=0.65))
    people = 0
    for a, b in zip(plain, drawn):
        assert a.rendered is None
        for f in FIELDS:
            assert np.array_equal(getattr(a, f), getattr(b, f)), f                 # the results are unchanged
        assert np.array_equal(b.rendered, a.plot_connections("limb", 0.65))        # the frame equals a separate render
        assert np.array_equal(b.rendered, _expected_frame(a, "limb", 0.65))
        people += len(a.kpts_coords)
    print("people drawn:", people)
    sized = model.infer_images(images[:2], max_batch=2, render=dict(bgr=True, out_height=64))
    for a, b in zip(plain, sized):
        h, w = a.raw_image.shape[:2]
        assert np.array_equal(b.rendered, cv_resize.resize(_expected_frame(a, "person", 0.8)[..., ::-1], (int(64 * w / h), 64)))
    with pytest.raises(ValueError):
        model.infer_images(images[:1], render=dict(colour="limb"))


@pytest.mark.parametrize("h,w", [(1280, 200), (640, 150), (300, 260)])  # the exact-2 path, no resize, the bilinear path
def test_video_frame(model, h, w):
    image = np.random.RandomState(h).randint(0, 255, (h, w, 3)).astype(np.uint8)
    res, out = model.video_frame(image)
    direct = model(image, None)
    for f in FIELDS:
        assert np.array_equal(getattr(res, f), getattr(direct, f)), f
    order = np.argsort(res.kpts_tags.mean(axis=1)[:, 0])
    drawn = _expected_frame(res, "limb", 0.65, order)[..., ::-1]
    new_w = int(640 * w / h)
    want = np.ascontiguousarray(drawn) if h == 640 else cv_resize.resize(np.ascontiguousarray(drawn), (new_w, 640))
    print("people:", len(res.kpts_coords))
    assert out.dtype == np.uint8 and out.shape == (640, new_w, 3) and np.array_equal(out, want)


@pytest.mark.parametrize("channels", [3, 1])
def test_resize_u8(vis, channels):
    for (h, w), (H, W) in (((1, 1), (3, 5)), ((7, 5), (7, 5)), ((64, 48), (32, 24)), ((37, 53), (640, int(640 * 53 / 37))), ((64, 48), (32, 25)),
                           ((9, 1030), (5, 1027))):
        src = frame(h, w, 3) if channels == 3 else np.ascontiguousarray(frame(h, w, 3)[..., 0])
        got = vis.to_host(vis.resize_device(torch.from_numpy(src).to(DEV), W, H))
        want = cv_resize.resize(src, (W, H))
        assert got.shape == want.shape and np.array_equal(got, want), ((h, w), (H, W), channels)
