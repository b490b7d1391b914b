"""-m gpu: the text kernel (hh_text_labels_u8_batch) against its numpy restatement (tests/text_ref.py), byte for byte, untouched bytes
against the input, and the Python interface built on it: put_txt, video_frame(labels=...), infer_images(render=dict(labels=...)), the
classifier's plot() and plot_top_preds_batch.  Frame sizes and primitive counts are aimed at the kernel's tile, chunk and pixel group
(hh_text_config); everything is a few tiles large."""
import importlib

import numpy as np
import pytest
import torch

import cv_resize
import text_ref as tr
from conftest import PKG
from text_helpers import edge_cases, tx  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 0xA5


def _on_device(images, gap=5):
    """The images in ONE device buffer, `gap` guard bytes in front of, between and behind them (so the frames lie at odd addresses)
    -> (buffer, [view of image j], [(start, stop) of image j])."""
    spans, at = [], gap
    for im in images:
        spans.append((at, at + im.size))
        at += im.size + gap
    host = np.full(at, GUARD, np.uint8)
    for (a, b), im in zip(spans, images):
        host[a:b] = im.reshape(-1)
    buf = torch.from_numpy(host).to(DEV)
    return buf, [buf[a:b].view(im.shape) for (a, b), im in zip(spans, images)], spans


def _check(buf, spans, wants, names):
    got = buf.cpu().numpy()
    inside = np.zeros(len(got), bool)
    for (a, b), want, name in zip(spans, wants, names):
        assert np.array_equal(got[a:b].reshape(want.shape), want), (name, int((got[a:b].reshape(want.shape) != want).sum()))
        inside[a:b] = True
    assert (got[~inside] == GUARD).all(), "a guard byte between the frames changed"


@pytest.fixture(scope="module")
def cases(tx):
    """The edge tables with their references, computed once."""
    return [(name, img, table, tr.apply_table(img, table)) for name, img, table in edge_cases(tx, tx.text_config())]


def test_mixed_size_batch_in_one_launch(tx, cases):
    TH, TW, _, _ = tx.text_config()
    pick = [c for c in cases if c[0].startswith("put_txt_")]
    assert [c[1].shape[:2] for c in pick] == [(1, 1), (20, 30), (TH - 1, TW + 1), (TH + 1, TW - 1)]
    assert all(c[1].shape[1] * 3 % 4 for c in pick)  # no row length is a multiple of 4 bytes
    plain = tr.image(120, TH + 1, TW + 1)
    pick = pick[:2] + [("no_primitives", plain, np.zeros(0, tx.PRIM), plain)] + pick[2:]
    buf, frames, spans = _on_device([c[1] for c in pick])
    assert tx.put_txt_device(frames, [c[2] for c in pick]) is frames
    _check(buf, spans, [c[3] for c in pick], [c[0] for c in pick])
    assert sum((c[3] != c[1]).any() for c in pick) == 4


def test_edge_tables_single_launches(tx, cases):
    """Clipping on all four sides, glyphs straddling the right and bottom edges and at negative origins, the alphas, the order of
    two overlapping tables, a chunk boundary inside a tile, every glyph of every size class; the frames at byte offsets 0..3."""
    for k, (name, img, table, want) in enumerate(cases):
        buf, (frame,), spans = _on_device([img], gap=k % 4)
        tx.put_txt_device([frame], [table])
        _check(buf, spans, [want], [name])
    by_name = {c[0]: c for c in cases}
    assert not np.array_equal(by_name["order_tl_br"][3], by_name["order_br_tl"][3])
    # at alpha 0 the box leaves every byte as it was
    _, img, table, _ = by_name["alpha_0.0"]
    frame = torch.from_numpy(img).to(DEV)
    tx.put_txt_device([frame], [table[:1]])
    assert table["kind"][0] == tr.BOX and table["x1"][0] > table["x0"][0] and np.array_equal(frame.cpu().numpy(), img)


def test_put_txt_takes_arrays_and_device_tensors(pkg, tx):
    img = tr.image(9, 90, 150)
    labels = ["put_txt", "on the device"]
    want = tr.put_txt(img, labels, loc="br", alpha=0.8, txt_color=(80, 255, 80))
    host = img.copy()
    assert pkg.keypoints.put_txt(host, labels, loc="br", alpha=0.8, txt_color=(80, 255, 80)) is host and np.array_equal(host, want)
    dev = torch.from_numpy(img).to(DEV)
    assert pkg.keypoints.put_txt(dev, labels, 10, None, 0.5, 1, "br", tr.GRAY, (80, 255, 80), 0.8) is dev and np.array_equal(dev.cpu().numpy(), want)


@pytest.fixture(scope="module")
def model(pkg):
    net = pkg.HigherHRNet(17, 32)
    net.load_state_dict({k: torch.from_numpy(pkg.synth.synth_param(k, v.shape, 3)) for k, v in net.state_dict().items()})
    return pkg.InferenceKeypointsModel(net.to(DEV).eval(), det_thr=0.05, tag_thr=0.5, use_flip=False, input_size=128, device=DEV)


def _video(frame, labels):
    return tr.put_txt(frame, labels, loc="tl", alpha=0.6, font_scale=0.5)


@pytest.mark.parametrize("h,w", [(640, 150), (300, 260)])  # no resize and a box wider than the frame; the bilinear path
def test_video_frame_labels(pkg, tx, model, h, w):
    image = np.random.RandomState(h).randint(0, 255, (h, w, 3)).astype(np.uint8)
    _, plain = model.video_frame(image)
    labels = tx.video_labels(3, 250, model.model_input_shape, {"preprocess": 2, "model": 19, "postprocess": 4})
    res, out = model.video_frame(image, labels=labels)
    want = _video(plain, labels)
    assert out.shape == plain.shape and np.array_equal(out, want) and (want != plain).any()
    assert np.array_equal(model.video_frame(image, labels=None)[1], plain)
    # the jpeg route: the labelled frame is encoded where it lies
    jp = pkg.keypoints.jpeg
    data = model.video_frame(image, jpeg=dict(quality=90, subsampling="420"), labels=labels)[1]
    assert isinstance(data, bytes) and data == jp.encode_jpeg_host(want, 90, "420", bgr=True)
    assert model.video_frame(image, jpeg=dict(quality=90, subsampling="420"))[1] == jp.encode_jpeg_host(plain, 90, "420", bgr=True)


def test_infer_images_render_labels(model):
    rs = np.random.RandomState(4)
    images = [rs.randint(0, 255, s + (3,)).astype(np.uint8) for s in ((64, 80), (70, 64))]
    labels = [["0 / 2", "Model input shape: 128 x 160"], ["1 / 2"]]
    plain = model.infer_images(images, max_batch=2, render=dict(color_mode="limb", alpha=0.65, out_height=96))
    drawn = model.infer_images(images, max_batch=2, render=dict(color_mode="limb", alpha=0.65, out_height=96, labels=labels))
    for a, b, lines in zip(plain, drawn, labels):
        assert a.rendered.shape[0] == 96 and np.array_equal(b.rendered, _video(a.rendered, lines)) and (b.rendered != a.rendered).any()
    skipped = model.infer_images(images, max_batch=2, render=dict(color_mode="limb", alpha=0.65, out_height=96, labels=[None, labels[1]]))
    assert np.array_equal(skipped[0].rendered, plain[0].rendered) and np.array_equal(skipped[1].rendered, drawn[1].rendered)
    with pytest.raises(ValueError, match="labels"):
        model.infer_images(images, render=dict(labels=[["one list for two images"]]))


def test_classifier_plots(pkg):
    cls = importlib.import_module(PKG + ".classification")
    vz = importlib.import_module(PKG + ".keypoints.visualization")
    net = pkg.ClassificationHRNet(32, 1000)
    net.load_state_dict({k: torch.from_numpy(pkg.synth.synth_param(k, v.shape, 3)) for k, v in net.state_dict().items()})
    idx2label = {i: f"class-{i}" for i in range(1000)}
    model = cls.InferenceClassificationModel(net, idx2label, input_size=64, device=DEV)
    rs = np.random.RandomState(2)
    images = [rs.randint(0, 256, (64, w, 3)).astype(np.uint8) for w in (24, 40, 64)]  # shorter sides 192, 320, 512 at height 512
    targets = ["class-7 with a target label wider than the image", None, 3]
    records = [model(im, t) for im, t in zip(images, targets)]
    wants = []
    for r, im, t, side in zip(records, images, targets, (192, 320, 512)):
        e = np.exp(r.logits)
        big = cv_resize.resize(im, (int(512 * im.shape[1] / 64), 512))
        assert min(big.shape[:2]) == side
        wants.append(tr.plot_top_preds(big, e / np.sum(e), idx2label, 5, t))
        plots = r.plot()
        assert set(plots) == {"top_preds"} and np.array_equal(plots["top_preds"], wants[-1]) and (wants[-1] != big).any()
    for got, want in zip(cls.plot_top_preds_batch(records), wants):
        assert np.array_equal(got, want)
    assert np.array_equal(cls.plot_top_preds(images[2], records[2].probs, idx2label, k=3, target_label="x"),
                          tr.plot_top_preds(images[2], records[2].probs, idx2label, 3, "x"))
    jp = pkg.keypoints.jpeg
    assert records[1].plot_jpeg()["top_preds"] == jp.encode_jpeg_host(wants[1], 90, "444")
    # the validation result: + eps in the softmax, the un-normalised model input
    x = model.prepare_input(images[2])
    res = cls.ClassificationResult(records[2].logits, 3, records[2].prediction, "three", x[0], idx2label)
    e = np.exp(res.logits) + np.finfo(res.logits.dtype).eps
    shown = vz.to_host(vz.unnormalize_device(x[0]))
    plots = res.plot()
    assert set(plots) == {"top_probs"} and np.array_equal(plots["top_probs"], tr.plot_top_preds(shown, e / np.sum(e), idx2label, 5, "three"))
    with pytest.raises(ValueError, match="model_input_image"):
        cls.ClassificationResult(res.logits, 3, 3).plot()
