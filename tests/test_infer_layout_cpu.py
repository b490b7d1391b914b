"""`infer_images` without a GPU: `batch_layout` and `jpeg.JpegBatch` against the byte layouts `infer_images`, `TrainInput.build` and
`ClsInput.build` had when each did its own arithmetic (every formula written out here, none computed through `Layout`), the invariants
of the device-only tail, and every refusal of `check_options` and `plan_batches` with its message."""
import importlib

import numpy as np
import pytest

from conftest import PKG
from test_jpeg_decode_cpu import corpus

WHOLE = ["420_120x200_scene_q90_plain", "422_21x43_scene_q90_plain", "444_17x23_scene_q90_plain"]
CLS = ["420_120x200_scene_q90_plain", "420_120x200_scene_q90_rows1", "422_21x43_scene_q90_plain", "444_17x23_scene_q90_plain", "400_17x23_scene_q90_plain",
       "420_33x50_noise_q75_plain"]  # the batch of tests/test_gpu_jpeg_window.py
MAX_BATCH = 32


@pytest.fixture(scope="module")
def ip(pkg):
    return importlib.import_module(PKG + ".keypoints._infer_pipeline")


@pytest.fixture(scope="module")
def J(pkg):
    return importlib.import_module(PKG + ".keypoints.jpeg")


def a64(x):
    return (x + 63) // 64 * 64


def a16(x):
    return (x + 15) // 16 * 16


def array(h, w):
    return np.zeros((h, w, 3), np.uint8)


def batches(J):
    """name -> (images, scales)"""
    three = [array(5, 7), array(96, 128), array(33, 1)]
    host, dev = J.JpegImage(corpus()[WHOLE[0]][0]), J.JpegImage(corpus()[WHOLE[1]][0], index="device")
    return {"one 1x1": ([array(1, 1)], 1), "three arrays": (three, 1), "three arrays, two scales": (three, 2),
            "two arrays and two JPEG items": ([array(5, 7), host, array(33, 1), dev], 1),
            "two arrays and two JPEG items, three scales": ([dev, array(5, 7), host, array(33, 1)], 3),
            "JPEG items only": ([host, dev, J.JpegImage(corpus()[WHOLE[2]][0])], 1),
            "max_batch of one size": ([array(48, 64)] * MAX_BATCH, 1)}


def device_tail(jb, start: int, end: int, sizes: list) -> list:
    """The invariants of the device-only part of a JpegBatch -> its sections [(first byte, past the last)]: the statuses 4-aligned with an
    int32 per item and call, every pixel slot 16-aligned with room for its pixels, all inside [start, end)."""
    assert jb.status_at % 4 == 0 and all(at % 16 == 0 for at in jb.pixel_at)
    sections = [(jb.status_at, jb.status_at + 4 * len(jb) * jb.calls)] + [(at, at + size) for at, size in zip(jb.pixel_at, sizes)]
    assert all(start <= a and b <= end for a, b in sections)
    return sections


def disjoint(sections: list) -> None:
    sections = sorted(s for s in sections if s[1] > s[0])
    assert all(a[1] <= b[0] for a, b in zip(sections[:-1], sections[1:])), sections


@pytest.mark.parametrize("name", ["one 1x1", "three arrays", "three arrays, two scales", "two arrays and two JPEG items",
                                  "two arrays and two JPEG items, three scales", "JPEG items only", "max_batch of one size"])
def test_batch_layout_is_the_layout_infer_images_had(ip, J, name):
    images, S = batches(J)[name]
    nb = len(images)
    items = [img for img in images if isinstance(img, J.JpegImage)]
    # the arithmetic infer_images did inline
    offs = np.cumsum([0] + [0 if isinstance(img, J.JpegImage) else img.size for img in images])
    desc_off = a64(int(offs[-1]))
    total = desc_off + 64 * nb * S
    if items:
        jdesc_off = a16(total)
        places = jdesc_off + 64 * len(items) + np.cumsum([0] + [it.staged_bytes() for it in items])
        total = int(places[-1])

    lay = ip.batch_layout(images, S)
    assert lay.upload == total and lay.device_total >= lay.upload
    assert lay.offs.tolist() == offs.tolist() and lay.desc_off == desc_off and lay.scale_desc == [desc_off + 64 * nb * si for si in range(S)]
    assert lay.jpeg_at == [j for j, img in enumerate(images) if isinstance(img, J.JpegImage)] and len(lay.jpegs) == len(items)
    assert ip._IMAGE_DESC.itemsize == 64 and J.DEC_DESC.itemsize == 64
    sections = [(int(offs[j]), int(offs[j + 1])) for j in range(nb)] + [(at, at + 64 * nb) for at in lay.scale_desc]
    assert desc_off % 64 == 0
    if items:
        jb = lay.jpegs
        assert jb.desc_at == jdesc_off and jb.places == places[:-1].tolist() and jb.desc_at % 16 == 0 and all(p % 16 == 0 for p in jb.places)
        sections += [(jb.desc_at, jb.desc_at + 64 * len(items))] + [(p, p + it.staged_bytes()) for p, it in zip(jb.places, items)]
        assert all(b <= lay.upload for _, b in sections)
        sections += device_tail(jb, lay.upload, lay.device_total, [it.h * it.w * 3 for it in items])
        assert jb.calls == (2 if any(it.device_index for it in items) else 1)
    else:
        assert lay.device_total == lay.upload
    disjoint(sections)
    # where the preprocess launch finds image j: its shipped pixels, or the slot the decode fills
    slots = iter(lay.jpegs.pixel_at)
    assert lay.pixel_at == [next(slots) if isinstance(img, J.JpegImage) else int(offs[j]) for j, img in enumerate(images)]


@pytest.mark.parametrize("front", [0, 1234, 4096 + 8 * 3])
@pytest.mark.parametrize("count", [0, 1, 3])
def test_jpeg_batch_whole_images_against_the_train_input_formula(pkg, J, front, count):
    """TrainInput.build: the section starts at align16(the end of the crowd tables), DEC_DESC.itemsize * J of descriptors, the blocks
    behind them; total = places[-1] with an item, unchanged without."""
    st = importlib.import_module(PKG + "._stage")
    items = [J.JpegImage(corpus()[n][0]) for n in WHOLE[:count]]
    jpeg_off = a16(front)
    places = jpeg_off + J.DEC_DESC.itemsize * count + np.cumsum([0] + [it.staged_bytes() for it in items])
    total = int(places[-1]) if items else front

    jb = J.JpegBatch(items, what="test")
    lay = st.Layout(front)
    jb.place_upload(lay)
    assert lay.end == total and len(jb) == count
    tail = a64(total) + 12345  # (the canvases and the filled masks lie between: the tail starts wherever the caller's other sections end)
    lay.end = tail
    jb.place_device(lay)
    if not items:
        assert lay.end == tail and jb.pixel_at == [] and jb.launch(None) is None
        jb.fill(np.zeros(0, np.uint8))
        return
    assert jb.desc_at == jpeg_off and jb.places == places[:-1].tolist() and jb.calls == 1 and jb.index_mps is None
    sections = device_tail(jb, tail, lay.end, [it.h * it.w * 3 for it in items])
    disjoint(sections + [(jb.desc_at, jb.desc_at + 64 * count)] + [(p, p + it.staged_bytes()) for p, it in zip(jb.places, items)])
    # the pinned bytes: every stream at its place, one descriptor row and one info per item
    hview = np.zeros(total, np.uint8)
    jb.fill(hview)
    assert jb.descs.dtype == J.DEC_DESC and len(jb.descs) == count == len(jb.infos)
    for p, it in zip(jb.places, items):
        assert np.array_equal(hview[p:p + it.data.size], it.data)


def test_jpeg_batch_windows_against_the_cls_input_formula(pkg, J):
    """ClsInput.build: the section starts at align16(target_off + 8 B), align16(WIN_DESC.itemsize * J) of descriptors, the plans'
    staged_bytes behind them; for the all-JPEG batch of tests/test_gpu_jpeg_window.py that is the figure pinned there."""
    st = importlib.import_module(PKG + "._stage")
    inp = importlib.import_module(PKG + ".classification.input")
    S = 16
    ci = inp.ClsInput(S, device="cpu")  # (nothing here touches a device)
    params = [inp.CropParams(40, 70, 30, 40, True), inp.inference_geometry(120, 200, resize=S + 4, crop=S), inp.CropWindow(3, 16, 17, 20, S + 3, S + 5, 2, 1, True, False),
              inp.CropParams(0, 0, 17, 23), inp.CropParams(16, 22, 1, 1, True), inp.CropWindow(15, 15, 18, 33, 2 * S, S, S // 2, 0)]
    items = [J.JpegImage(corpus()[n][0]) for n in CLS]
    windows = [ci.window(it.h, it.w, p) for it, p in zip(items, params)]
    plans = [it.window_plan((q.top, q.left, q.height, q.width)) for it, q in zip(items, windows)]
    for lo, hi, B in ((0, 6, 6), (1, 4, 7), (5, 6, 1)):  # the items [lo, hi) among B samples, the others arrays of 3 x 5 pixels
        pixels = 3 * 5 * 3 * (B - (hi - lo))
        target_off = a64(pixels) + 56 * B
        jpeg_off = a16(target_off + 8 * B)
        places = jpeg_off + a16(J.WIN_DESC.itemsize * (hi - lo)) + np.cumsum([0] + [p.staged_bytes for p in plans[lo:hi]])
        assert ci.layout([(0, 0)] * (hi - lo) + [(3, 5)] * (B - (hi - lo)))[3] == target_off + 8 * B

        jb = J.JpegBatch(items[lo:hi], plans[lo:hi], "test")
        lay = st.Layout(target_off + 8 * B)
        jb.place_upload(lay)
        upload = lay.end
        assert jb.windowed and jb.desc_t == J.WIN_DESC and J.WIN_DESC.itemsize == 80
        assert upload == int(places[-1]) and jb.desc_at == jpeg_off and jb.places == places[:-1].tolist()
        if (lo, hi, B) == (0, 6, 6):
            assert upload == (56 * 6 + 8 * 6 + 15) // 16 * 16 + 80 * 6 + sum(p.staged_bytes for p in plans)
        jb.place_device(lay)
        sections = device_tail(jb, upload, lay.end, [q.height * q.width * 3 for q in windows[lo:hi]])
        disjoint(sections + [(jb.desc_at, jb.desc_at + 80 * (hi - lo))] + [(at, at + p.staged_bytes) for at, p in zip(jb.places, plans[lo:hi])])
        hview = np.zeros(upload, np.uint8)
        jb.fill(hview)
        assert jb.descs.dtype == J.WIN_DESC and len(jb.descs) == hi - lo == len(jb.infos)
        for at, it, p in zip(jb.places, items[lo:hi], plans[lo:hi]):
            assert np.array_equal(hview[at:at + p.slice[1] - p.slice[0]], it.data[p.slice[0]:p.slice[1]])


def test_jpeg_batch_refuses_two_index_granularities(J):
    data = corpus()[WHOLE[0]][0]
    with pytest.raises(ValueError, match=r"infer_images: the device-indexed images of one batch must share one mcus_per_segment, got \[2, 5\]"):
        J.JpegBatch([J.JpegImage(data, index="device", mcus_per_segment=2), J.JpegImage(data, index="device", mcus_per_segment=5)], what="infer_images")
    one = J.JpegBatch([J.JpegImage(data, index="device", mcus_per_segment=2), J.JpegImage(data)], what="infer_images")
    assert one.index_mps == 2 and one.calls == 2
    assert one.codes(np.array([0, 3, 1, 0], np.int32)).tolist() == [1, 3]  # per item the larger of the decode's and the index call's code


class _Tracker:
    def __init__(self, streams):
        self.streams, self.bound = streams, None

    def bind_input_shape(self, shape):
        self.bound = tuple(shape)


def test_check_options_refuses_by_name(ip, pkg):
    ps = importlib.import_module(PKG + ".keypoints.pose_score")
    check = ip.check_options
    with pytest.raises(ValueError, match=r"^infer_images: render color_mode 'track' needs a tracker$"):
        check(dict(color_mode="track"), None, None, 2, 17, 30)
    with pytest.raises(ValueError, match=r"^infer_images: unknown render option\(s\) \['colour', 'thickness'\]$"):
        check(dict(alpha=0.5, thickness=2, colour=1), None, None, 2, 17, 30)
    with pytest.raises(ValueError, match=r"^infer_images: render labels: one list of strings \(or None\) per image$"):
        check(dict(labels=[["a"]]), None, None, 2, 17, 30)
    with pytest.raises(ValueError, match=r"^infer_images: score must be None, 'oks' or 'pckh', got 'ap'$"):
        check(None, None, "ap", 2, 17, 30)
    with pytest.raises(ValueError, match=rf"^infer_images: score= takes at most HH_POSE_MAX_P \({ps.MAX_P}\) people per image, the parser keeps {ps.MAX_P + 1}$"):
        check(None, None, "pckh", 2, 17, ps.MAX_P + 1)
    with pytest.raises(ValueError, match=r"^pose_score: the OKS constants are those of the 17 COCO keypoints, not of 16: pass your own variances"):
        check(None, None, "oks", 2, 16, 30)
    # what passes, and what it gives
    assert check(None, None, None, 0, 16, 1000) is None
    assert check(dict(color_mode="track", alpha=0.65, bgr=True, out_height=64, jpeg=dict(quality=80), labels=[None, ["a"]]), _Tracker(1), None, 2, 17, 30) is None
    assert np.array_equal(check(None, None, "oks", 2, 17, ps.MAX_P), ps.OKS_VARIANCES) and np.array_equal(check(None, None, "pckh", 2, 16, 30), np.ones(16))


def test_plan_batches_refuses_by_name_and_buckets(ip):
    # (the short side goes to 128, the long one up to the next multiple of 64: 96 x 128 -> 128 x 192)
    wide, tall = [array(96, 128)] * 3, [array(128, 96)]
    with pytest.raises(ValueError, match=r"^infer_images: the tracker must have one stream \(the images are one clip\)$"):
        ip.plan_batches(wide, 128, None, 2, _Tracker(2))
    with pytest.raises(ValueError, match=r"^infer_images: the frames of a tracked clip must share one model-input shape, got \(w, h\) = \[\(128, 192\), \(192, 128\)\]$"):
        ip.plan_batches(wide + tall, 128, None, 2, _Tracker(1))
    with pytest.raises(ValueError, match=r"^plan_multi_scale: scales must contain 1.0"):
        ip.plan_batches(wide, 128, (0.5, 2.0), 2)
    tracker = _Tracker(1)
    plan = ip.plan_batches(wide, 128, None, 2, tracker)
    assert tracker.bound == (128, 192) and plan.scales == (1,) and plan.i1 == 0 and len(plan.geo) == 3
    assert plan.jobs == [(((192, 128),), [0, 1], None), (((192, 128),), [2], None)]  # three frames, max_batch 2: the last batch is short
    assert ip.plan_batches([], 128, None, 2, _Tracker(2)).jobs == []  # (no image: nothing is asked of the tracker)
    mixed = ip.plan_batches([wide[0], tall[0], wide[0]], 128, None, 8)
    assert [(sizes, chunk) for sizes, chunk, _ in mixed.jobs] == [(((192, 128),), [0, 2]), (((128, 192),), [1])]
    multi = ip.plan_batches(wide, 128, (0.5, 1.0), 2)
    assert multi.scales == (0.5, 1.0) and multi.i1 == 1 and [chunk for _, chunk, _ in multi.jobs] == [[0, 1], [2]]
    assert all(len(sizes) == 2 and len(subs) == 2 for sizes, _, subs in multi.jobs)
