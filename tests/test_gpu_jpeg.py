"""hh_jpeg_encode_u8_batch on the GPU against the same rule compiled for the host (hh_debug_jpeg_encode_host, itself held byte for byte
against the numpy restatement and Pillow's decoder by tests/test_jpeg_cpu.py): streams and lengths equal, lengths within the bound, over
the sizes at which the kernels take another path; every refusal; the hooks of the inference API."""
import importlib

import numpy as np
import pytest
import torch

from conftest import PKG
from test_gpu_render import model  # noqa: F401
from test_jpeg_cpu import picture

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def J(pkg):
    return importlib.import_module(PKG + ".keypoints.jpeg")


def _check(J, frames, streams, quality, sub, bgr=False):
    for f, s in zip(frames, streams):
        arr = f.cpu().numpy() if isinstance(f, torch.Tensor) else f
        want = J.encode_jpeg_host(arr, quality, sub, bgr)
        assert len(s) == len(want) <= J.jpeg_bound(arr.shape[0], arr.shape[1], sub)
        assert s == want, next(i for i, (a, b) in enumerate(zip(s, want)) if a != b)


@pytest.mark.parametrize("h,w,sub,content,quality", [
    (8, 8, 444, "scene", 90),      # one MCU
    (8, 8, 420, "scene", 90),      # padded in both axes
    (17, 23, 420, "scene", 75),    # edge replication
    (17, 23, 444, "noise", 30),
    (33, 50, 420, "noise", 90),
    (33, 50, 444, "scene", 1),
    (130, 24, 420, "scene", 90),   # 9 MCU rows: RSTm wraps
    (24, 40, 420, "flat", 90),     # every AC zero, every DC difference zero
    (24, 40, 444, "flat", 100),
])
def test_device_stream_equals_host_stream(J, h, w, sub, content, quality):
    img = picture(content, h, w)
    for frame in (img, torch.from_numpy(img).to(DEV)):  # uploaded through the pinned block; read in place
        _check(J, [img], J.encode_jpeg_device([frame], quality, sub), quality, sub)


def test_long_interval_with_worst_case_codes(J):
    """16 x 1120 noise at quality 100, 4:2:0: one interval of 420 blocks, seven passes of 64 lanes with the partial byte carried across,
    long codes, stuffed bytes."""
    img = picture("noise", 16, 1120)
    (got,) = J.encode_jpeg_device([torch.from_numpy(img).to(DEV)], 100, 420)
    _check(J, [img], [got], 100, 420)
    assert got[629:].count(b"\xff\x00") > 0
    assert len(got) - 629 > 64 * 64  # (the interval is long: several passes leave more than 4 KB)


def test_mixed_batch_equals_single_calls(J):
    imgs = [picture("scene", 33, 50), picture("noise", 17, 23), picture("scene", 130, 24), picture("flat", 8, 8), picture("noise", 64, 96)]
    quals, subs, bgrs = [90, 100, 30, 75, 1], [420, 444, 420, 444, 420], [False, True, False, False, False]
    wide = torch.full((64, 101, 3), 9, dtype=torch.uint8, device=DEV)
    wide[:, :96] = torch.from_numpy(imgs[4]).to(DEV)
    frames = [torch.from_numpy(imgs[0]).to(DEV), imgs[1], torch.from_numpy(imgs[2]).to(DEV), imgs[3], wide[:, :96]]  # the last: a pitched view
    assert frames[4].stride(0) == 303 and not frames[4].is_contiguous()
    got = J.encode_jpeg_device(frames, quals, subs, bgrs)
    for j in range(5):
        single = J.encode_jpeg_device([frames[j]], quals[j], subs[j], bgrs[j])[0]
        assert got[j] == single
        _check(J, [imgs[j]], [got[j]], quals[j], subs[j], bgrs[j])


def test_first_use_on_a_fresh_stream(J):
    img = picture("scene", 33, 50)
    side = torch.cuda.Stream(DEV)  # (non-blocking: it does not synchronise with the null stream)
    with torch.cuda.stream(side):
        got = J.encode_jpeg_device([img], 90, 420)
    _check(J, [img], got, 90, 420)


def test_every_refusal_launches_nothing(J, pkg):
    """The library refuses before any launch: the 0xA5 output and the lengths are untouched."""
    lib, HHError = pkg._lib.load(), pkg._lib.HHError
    h, w = 16, 24
    img = torch.from_numpy(picture("scene", h, w)).to(DEV)
    cap, ws = J.jpeg_bound(h, w, 420), J.workspace_bytes(h, w, 420)
    out = torch.full((cap,), 0xA5, dtype=torch.uint8, device=DEV)
    work = torch.empty(ws, dtype=torch.uint8, device=DEV)
    lengths = torch.full((1,), -7, dtype=torch.int32, device=DEV)
    descs_dev = torch.zeros(64, dtype=torch.uint8, device=DEV)
    base = min(img.data_ptr(), out.data_ptr())

    def call(quality=90, sub=420, pitch=3 * w, capacity=cap, ws_bytes=ws):
        desc = np.zeros(1, J.DESC)
        desc[0] = (img.data_ptr() - base, out.data_ptr() - base, capacity, 0, pitch, h, w, quality, sub, 0, 0)
        descs_dev.copy_(torch.from_numpy(desc.view(np.uint8)))
        pkg._lib.launch(img.device, lib.hh_jpeg_encode_u8_batch, base, descs_dev.data_ptr(), desc.ctypes.data, 1, work.data_ptr(), ws_bytes,
                        lengths.data_ptr())

    for kwargs, message in ((dict(quality=0), "quality outside 1..100"), (dict(quality=101), "quality outside 1..100"),
                            (dict(sub=422), "subsampling must be 420 or 444"), (dict(pitch=3 * w - 1), "pitch below 3 \\* w"),
                            (dict(capacity=cap - 1), "output capacity below hh_jpeg_bound"), (dict(ws_bytes=ws - 1), "workspace below")):
        with pytest.raises(HHError, match=message):
            call(**kwargs)
    torch.cuda.synchronize()
    assert bool((out == 0xA5).all()) and int(lengths[0]) == -7
    call()  # the same call, accepted
    torch.cuda.synchronize()
    n = int(lengths[0])
    assert out[:n].cpu().numpy().tobytes() == J.encode_jpeg_host(img.cpu().numpy(), 90, 420) and bool((out[n:] == 0xA5).all())
    # the Python surface refuses the same by name
    for kwargs, message in ((dict(quality=0), "quality outside 1..100"), (dict(subsampling="422"), "subsampling must be 420 or 444"),
                            (dict(capacity=cap - 1), "output capacity below hh_jpeg_bound")):
        with pytest.raises(HHError, match=message):
            J.encode_jpeg_device([img], **kwargs)


# ---------------------------------------------------------------- hooks
def test_video_frame_jpeg(J, model):  # noqa: F811
    image = np.random.RandomState(300).randint(0, 255, (300, 260, 3)).astype(np.uint8)
    _, frame = model.video_frame(image)
    res, data = model.video_frame(image, jpeg=dict(quality=80, subsampling="420"))
    assert isinstance(data, bytes) and frame.shape[0] == 640
    assert data == J.encode_jpeg_host(frame, 80, 420, bgr=True)
    assert len(data) < frame.size // 2


def test_infer_images_render_jpeg(J, model):  # noqa: F811
    rs = np.random.RandomState(9)
    images = [rs.randint(0, 255, s + (3,)).astype(np.uint8) for s in [(150, 220), (128, 128)]]
    raw = model.infer_images(images, max_batch=2, render=dict(color_mode="limb", alpha=0.65, bgr=True))
    enc = model.infer_images(images, max_batch=2, render=dict(color_mode="limb", alpha=0.65, bgr=True, jpeg=dict(quality=90, subsampling="420")))
    for a, b in zip(raw, enc):
        assert a.rendered_jpeg is None and b.rendered is None
        assert b.rendered_jpeg == J.encode_jpeg_host(a.rendered, 90, 420, bgr=True)


def test_plot_jpeg(J, pkg, model):  # noqa: F811
    image = np.random.RandomState(5).randint(0, 255, (150, 220, 3)).astype(np.uint8)
    res = model(image, None)
    plots, enc = res.plot(), res.plot_jpeg()
    assert set(enc) == set(plots) == {"connections", "heatmaps"}
    for name in plots:
        assert enc[name] == J.encode_jpeg_host(plots[name], 90, 444)
    vres = pkg.keypoints.KeypointsResult(res.model_input_image.cpu(), [h[:1] for h in res._stage_hms], res._tags[0][:1], res.limbs, 20, 0.1, 1.0)
    vres.set_preds()
    plots, enc = vres.plot(), vres.plot_jpeg(quality=75, subsampling="420")
    assert set(enc) == set(plots) == {"heatmaps"} and enc["heatmaps"] == J.encode_jpeg_host(plots["heatmaps"], 75, 420)
