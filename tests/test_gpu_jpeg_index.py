"""hh_jpeg_index_device_batch on the GPU: the entries it writes into the table blocks against hh_jpeg_index_host's (build_jpeg_index), bit
for bit, and the pixels decoded through them against Pillow's (tests/golden/jpeg_decode.npz) and the host rule's; several rounds of
1024 lanes; batches that mix device-indexed, host-indexed and DRI streams; the status path; a fresh stream; and
InferenceKeypointsModel.infer_images / __call__ fed JPEG bytes against the same calls fed Pillow's arrays
(tests/test_jpeg_index_sync_cpu.py holds the host twin of the kernel against the same yardstick)."""
import functools
import importlib
import io

import numpy as np
import pytest
import torch

from conftest import PKG
from test_jpeg_decode_cpu import bad_code_stream, corpus, names, truncated_stream

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def J(pkg):
    return importlib.import_module(PKG + ".keypoints.jpeg")


@functools.lru_cache(maxsize=None)
def restartless() -> tuple:
    J = importlib.import_module(PKG + ".keypoints.jpeg")
    return tuple(n for n in names() if not J.jpeg_info(corpus()[n][0]).restart_interval)


def assert_entries(J, got, data, mps, where):
    want = J.build_jpeg_index(data, mps)
    assert got.dtype == want.dtype and len(got) == len(want), where
    assert got.tobytes() == want.tobytes(), (where, [i for i in range(len(want)) if got[i] != want[i]][:3])


@pytest.mark.parametrize("subseq", ["minimum", 128, None])  # (None: the default, 32)
@pytest.mark.parametrize("mps", [1, 2, "row"])
def test_corpus_as_one_batch(J, mps, subseq):
    use = restartless()
    assert len(use) >= 40
    sub = J.index_config()[2] if subseq == "minimum" else subseq
    # (one index call has one mcus_per_segment: "one MCU row" is a call per row length)
    groups = {}
    for n in use:
        groups.setdefault(J.jpeg_info(corpus()[n][0]).mcu_cols if mps == "row" else mps, []).append(n)
    for size, batch in groups.items():
        entries = []
        got = J.decode_jpeg_device([corpus()[n][0] for n in batch], "device", device=DEV, mcus_per_segment=size, subseq_bytes=sub, entries_out=entries)
        assert J.decode_jpeg_device.last_status.tolist() == [0] * len(batch)
        for n, g, e in zip(batch, got, entries):
            assert_entries(J, e, corpus()[n][0], size, (n, size, sub))
            assert np.array_equal(g.cpu().numpy(), corpus()[n][1]), (n, size, sub)


@functools.lru_cache(maxsize=None)
def large_noise_stream() -> bytes:
    Image = pytest.importorskip("PIL.Image")
    pixels = np.random.default_rng(3).integers(0, 256, (480, 640, 3), dtype=np.uint8)
    f = io.BytesIO()
    Image.fromarray(pixels, "RGB").save(f, "JPEG", quality=95, subsampling=2)
    return f.getvalue()


def test_several_rounds_on_the_device(J):
    data = large_noise_stream()
    info = J.jpeg_info(data)
    lanes = J.index_config()[0]
    assert 2 * lanes < -(-(info.scan_end - info.scan_offset) // 128) <= 3 * lanes  # three rounds at 128-byte subsequences, eleven at the default
    want = J.decode_jpeg_host(data)
    for mps, sub in ((2, 128), (info.mcu_cols, None)):
        entries = []
        (got,) = J.decode_jpeg_device([data], "device", device=DEV, mcus_per_segment=mps, subseq_bytes=sub, entries_out=entries)
        assert_entries(J, entries[0], data, mps, (mps, sub))
        assert np.array_equal(got.cpu().numpy(), want), (mps, sub)


MIXED = ["420_33x50_scene_q90_plain", "420_33x50_scene_q90_rows1", "422_21x43_noise_q90_plain", "444_17x23_noise_q30_plain", "400_17x23_scene_q90_plain",
         "420_130x24_scene_q90_own", "420_120x200_scene_q90_plain"]


def test_mixed_batch_equals_single_calls(J):
    """Device-indexed, host-indexed, DRI (given "device", and given nothing) and B,G,R streams in one batch."""
    streams = [corpus()[n][0] for n in MIXED]
    index = ["device", "device", J.build_jpeg_index(streams[2], 3), "device", None, None, "device"]
    bgr = [False, True, False, True, False, True, True]
    entries = []
    got = J.decode_jpeg_device(streams, index, bgr, device=DEV, entries_out=entries)
    assert J.decode_jpeg_device.last_status.tolist() == [0] * len(MIXED)
    for j, n in enumerate(MIXED):
        single = J.decode_jpeg_device([streams[j]], [index[j]], bgr[j], device=DEV)[0]
        want = corpus()[n][1][:, :, ::-1] if bgr[j] else corpus()[n][1]
        assert torch.equal(got[j], single) and np.array_equal(single.cpu().numpy(), want), n
    for j in (0, 3, 6):
        assert_entries(J, entries[j], streams[j], J.index_config()[3], MIXED[j])
    assert entries[1].tobytes() == J.JpegImage(streams[1]).segments.tobytes()  # DRI: its restart segments, untouched by the index launch
    assert entries[2].tobytes() == index[2].tobytes()


def test_malformed_streams_in_a_batch(J, pkg):
    """A truncated stream and one with a substituted byte, device-indexed among good ones: HHError names them with the codes
    hh_jpeg_index_host meets; the others decode, and nothing passes a slot's end."""
    cut, _ = truncated_stream(J)
    bad, _ = bad_code_stream(J, pkg)
    for data, code in ((cut, "bytes exhausted"), (bad, "bad Huffman code")):
        with pytest.raises(pkg._lib.HHError, match="the scan cannot be walked: " + code):
            J.build_jpeg_index(data, 2)
    good = ["420_33x50_scene_q90_rows1", "422_21x43_noise_q90_plain", "420_17x23_scene_q90_plain"]
    items = [J.JpegImage(corpus()[good[0]][0], "device"), J.JpegImage(cut, "device"), J.JpegImage(corpus()[good[1]][0], "device"), J.JpegImage(bad, "device"),
             J.JpegImage(corpus()[good[2]][0])]
    gap = 256
    offs = np.cumsum([0] + [it.h * it.w * 3 + gap for it in items])
    slab = torch.full((int(offs[-1]),), 0xA5, dtype=torch.uint8, device=DEV)
    out = [slab[int(o):int(o) + it.h * it.w * 3].view(it.h, it.w, 3) for o, it in zip(offs, items)]
    with pytest.raises(pkg._lib.HHError, match=r"image 1: status 3 \(bytes exhausted\); also images \[3\]"):
        J.decode_jpeg_device(items, device=DEV, out=out)
    assert J.decode_jpeg_device.last_status.tolist() == [0, 3, 0, 1, 0]
    for j, n in ((0, good[0]), (2, good[1]), (4, good[2])):
        assert np.array_equal(out[j].cpu().numpy(), corpus()[n][1]), n
    for o, it in zip(offs, items):
        assert bool((slab[int(o) + it.h * it.w * 3:int(o) + it.h * it.w * 3 + gap] == 0xA5).all())


def test_first_use_on_a_fresh_stream(J):
    side = torch.cuda.Stream(DEV)  # (non-blocking: it does not synchronise with the null stream)
    use = MIXED[:3]
    with torch.cuda.stream(side):
        got = J.decode_jpeg_device([corpus()[n][0] for n in use], "device", device=DEV)
    side.synchronize()
    for n, g in zip(use, got):
        assert np.array_equal(g.cpu().numpy(), corpus()[n][1])


FIELDS = ("kpts_coords", "kpts_scores", "kpts_tags", "obj_scores")
PICTURES = ["420_120x200_scene_q90_plain", "420_120x200_scene_q90_rows1", "420_36x44_noise_q90_plain", "420_120x200_scene_q90_plain",
            "422_21x43_scene_q90_plain", "420_33x50_scene_q90_plain"]


@pytest.fixture(scope="module")
def model(pkg):
    net = pkg.HigherHRNet(17, 32)
    net.load_state_dict({k: torch.from_numpy(pkg.synth.synth_param(k, v.shape, 3)) for k, v in net.state_dict().items()})
    return pkg.InferenceKeypointsModel(net.to(DEV).eval(), det_thr=0.05, tag_thr=0.5, use_flip=False, input_size=128, device=DEV)


def _same_results(got, want):
    assert len(got) == len(want)
    for a, b in zip(got, want):
        for f in FIELDS:
            x, y = getattr(a, f), getattr(b, f)
            assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y), f
        assert torch.equal(a.model_input_image, b.model_input_image)


def test_infer_images_from_bytes(J, pkg, model):
    """bytes (index on the device), JpegImage (DRI; host-indexed; device-indexed) and Pillow arrays of the same pictures in one list, in
    buckets that split, against the all-array call: bit-identical results, also multi-scale and rendered; __call__; .raw_image."""
    arrays = [corpus()[n][1] for n in PICTURES]
    data = [corpus()[n][0] for n in PICTURES]
    mixed = [data[0], J.JpegImage(data[1], index="device"), bytearray(data[2]), arrays[3], J.JpegImage(data[4]), memoryview(data[5])]
    want = model.infer_images(arrays, max_batch=2)
    array_bytes = model.last_h2d_bytes
    got = model.infer_images(mixed, max_batch=2)
    assert model.last_h2d_bytes < array_bytes
    _same_results(got, want)
    assert sum(len(r.kpts_coords) for r in want) > 0
    for r, a, m in zip(got, arrays, mixed):
        assert (r.raw_image is a) if isinstance(m, np.ndarray) else (r.raw_image is not m and np.array_equal(r.raw_image, a))
        assert r.raw_image is r.raw_image and r.raw_shape == a.shape
    _same_results(model.infer_images(mixed, max_batch=2, scales=(0.5, 1)), model.infer_images(arrays, max_batch=2, scales=(0.5, 1)))
    render = dict(color_mode="limb", alpha=0.65, bgr=True)
    drawn, drawn_want = model.infer_images(mixed, max_batch=4, render=render), model.infer_images(arrays, max_batch=4, render=render)
    _same_results(drawn, drawn_want)
    for a, b in zip(drawn, drawn_want):
        assert a.rendered.shape == b.rendered.shape and np.array_equal(a.rendered, b.rendered)
    one, one_want = model(data[0], None), model(arrays[0], None)
    _same_results([one], [one_want])
    assert np.array_equal(one.raw_image, arrays[0])
    # a stream that cannot be walked raises when its batch is collected, by name
    cut, _ = truncated_stream(J)
    with pytest.raises(pkg._lib.HHError, match=r"infer_images: image 1: its JPEG stream cannot be decoded: status 3 \(bytes exhausted\)"):
        model.infer_images([arrays[5], cut, data[5]], max_batch=4)
