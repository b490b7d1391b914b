"""hh_jpeg_decode_u8_batch on the GPU against the same rule compiled for the host (hh_debug_jpeg_decode_host) and against Pillow's pixels
of tests/golden/jpeg_decode.npz (tests/test_jpeg_decode_cpu.py holds host == numpy restatement == Pillow): byte for byte on every
corpus entry, a mixed batch, B,G,R, a pitched destination, a fresh stream, every launch-time refusal, the status path on two malformed
streams, JpegImage samples in TrainInput, MJPEGReader.read.  Pillow is not imported here."""
import importlib

import numpy as np
import pytest
import torch

from conftest import PKG
from test_gpu_crowd_mask import annotation, assert_same_batch
from test_jpeg_cpu import picture
from test_jpeg_decode_cpu import bad_code_stream, corpus, names, truncated_stream

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def J(pkg):
    return importlib.import_module(PKG + ".keypoints.jpeg")


def test_device_equals_host_equals_pillow_on_the_corpus(J):
    """Every entry, in batches of mixed entries (one call each): through the restart intervals where the stream has them, through an
    index built on the spot where it has none."""
    all_names = names()
    for first in range(0, len(all_names), 14):
        batch = all_names[first:first + 14]
        got = J.decode_jpeg_device([corpus()[n][0] for n in batch], device=DEV)
        for n, g in zip(batch, got):
            data, pixels = corpus()[n]
            assert g.dtype == torch.uint8 and tuple(g.shape) == pixels.shape, n
            assert np.array_equal(g.cpu().numpy(), pixels), n
            assert np.array_equal(J.decode_jpeg_host(data), pixels), n


@pytest.mark.parametrize("mps", [1, 3, None])
def test_decoding_through_an_index_of_any_segment_size(J, mps):
    batch = ["420_33x50_noise_q75_plain", "420_130x24_scene_q90_plain", "422_21x43_noise_q90_plain", "400_17x23_noise_q75_plain",
             "420_33x50_noise_q90_blocks3", "420_120x200_scene_q90_plain"]
    index = [J.build_jpeg_index(corpus()[n][0], mps) for n in batch]
    got = J.decode_jpeg_device([corpus()[n][0] for n in batch], index, device=DEV)
    for n, g in zip(batch, got):
        assert np.array_equal(g.cpu().numpy(), corpus()[n][1]), n


MIXED = ["420_33x50_scene_q90_rows1", "422_21x43_noise_q90_plain", "444_17x23_noise_q30_plain", "400_17x23_scene_q90_plain", "420_130x24_scene_q90_own"]


def test_mixed_batch_equals_single_calls_and_bgr(J):
    streams = [corpus()[n][0] for n in MIXED]
    got = J.decode_jpeg_device(streams, device=DEV)
    swapped = J.decode_jpeg_device(streams, bgr=[False, True, True, False, True], device=DEV)
    for j, n in enumerate(MIXED):
        single = J.decode_jpeg_device([streams[j]], device=DEV)[0]
        assert torch.equal(got[j], single) and np.array_equal(single.cpu().numpy(), corpus()[n][1])
        want = corpus()[n][1][:, :, ::-1] if j in (1, 2, 4) else corpus()[n][1]
        assert np.array_equal(swapped[j].cpu().numpy(), want), n
        assert np.array_equal(J.decode_jpeg_host(streams[j], bgr=j in (1, 2, 4)), want)


def test_pitched_destination_keeps_the_bytes_between_rows(J):
    name = "420_33x50_scene_q90_plain"
    data, pixels = corpus()[name]
    h, w = pixels.shape[:2]
    wide = torch.full((h, w + 7, 3), 0xA5, dtype=torch.uint8, device=DEV)
    view = wide[:, :w]
    assert view.stride(0) == 3 * (w + 7) and not view.is_contiguous()
    (out,) = J.decode_jpeg_device([data], device=DEV, out=[view])
    assert out.data_ptr() == wide.data_ptr()
    assert np.array_equal(wide[:, :w].cpu().numpy(), pixels) and bool((wide[:, w:] == 0xA5).all())


def test_first_use_on_a_fresh_stream(J):
    side = torch.cuda.Stream(DEV)  # (non-blocking: it does not synchronise with the null stream)
    with torch.cuda.stream(side):
        got = J.decode_jpeg_device([corpus()[n][0] for n in MIXED[:2]], device=DEV)
    side.synchronize()
    for n, g in zip(MIXED, got):
        assert np.array_equal(g.cpu().numpy(), corpus()[n][1])


def test_every_refusal_launches_nothing(J, pkg):
    """The library refuses before any launch or clearing: the 0xA5 destination and the statuses are untouched."""
    lib, HHError = pkg._lib.load(), pkg._lib.HHError
    data, pixels = corpus()["420_33x50_scene_q90_rows1"]
    item = J.JpegImage(data)
    h, w = item.h, item.w
    stage = np.zeros(64 + item.staged_bytes(), np.uint8)
    stream_at, tables_at = item.stage(stage, 64)
    buf = torch.from_numpy(stage).to(DEV)
    out = torch.full((h * w * 3 + 64,), 0xA5, dtype=torch.uint8, device=DEV)
    work = torch.empty(item.ws_bytes, dtype=torch.uint8, device=DEV)
    status = torch.full((1,), -7, dtype=torch.int32, device=DEV)
    base = min(buf.data_ptr(), out.data_ptr())
    rel, dst = buf.data_ptr() - base, out.data_ptr() - base

    def call(n=1, pitch=3 * w, ws_bytes=item.ws_bytes, tables_bytes=item.tables_bytes, dst_offset=dst, nseg=len(item.segments), flags=0, info=item.info):
        desc = np.zeros(1, J.DEC_DESC)
        desc[0] = (rel + stream_at, rel + tables_at, tables_bytes, dst_offset, 0, pitch, len(data), nseg, flags, 0)
        buf[:64].copy_(torch.from_numpy(desc.view(np.uint8)))
        pkg._lib.launch(buf.device, lib.hh_jpeg_decode_u8_batch, base, buf.data_ptr(), desc.ctypes.data, info.ctypes.data, n, work.data_ptr(), ws_bytes,
                        status.data_ptr())

    wrong = item.info.copy()
    wrong["mcols"] += 1
    for kwargs, message in ((dict(pitch=3 * w - 1), "pitch below 3 \\* w"), (dict(ws_bytes=item.ws_bytes - 1), "workspace below hh_jpeg_decode_workspace_bytes"),
                            (dict(tables_bytes=item.tables_bytes - 1), "table block below hh_jpeg_decode_tables_bytes"),
                            (dict(dst_offset=-1), "negative offset"), (dict(n=0), "need 1 <= n"), (dict(nseg=0), "nseg must be at least 1"),
                            (dict(flags=2), "unknown flag"), (dict(info=wrong), "bad stream info")):
        with pytest.raises(HHError, match=message):
            call(**kwargs)
    torch.cuda.synchronize()
    assert bool((out == 0xA5).all()) and int(status[0]) == -7
    call()  # the same call, accepted
    torch.cuda.synchronize()
    assert int(status[0]) == 0
    assert np.array_equal(out[:h * w * 3].view(h, w, 3).cpu().numpy(), pixels) and bool((out[h * w * 3:] == 0xA5).all())


def test_malformed_streams_raise_a_status_and_leave_the_rest_alone(J, pkg):
    """The status path, once: a stream cut inside its scan and one with a substituted scan byte (a bad code on the host), both of which
    tools/jpeg_decode_host_check.cpp's kind of input; only they fail, the batch's other images decode, and nothing passes a slot's end."""
    cut, cut_index = truncated_stream(J)
    bad, _ = bad_code_stream(J, pkg)
    good = ["420_33x50_scene_q90_rows1", "422_21x43_noise_q90_plain", "420_17x23_scene_q90_plain"]
    whole_index = J.build_jpeg_index(corpus()["420_33x50_noise_q75_plain"][0])
    items = [J.JpegImage(corpus()[good[0]][0]), J.JpegImage(cut, cut_index), J.JpegImage(corpus()[good[1]][0]), J.JpegImage(bad, whole_index),
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
    # the MCU rows in front of the cut are what the whole stream decodes to
    assert np.array_equal(out[1][:16].cpu().numpy(), corpus()["420_33x50_noise_q75_plain"][1][:16])


def _sample(pkg, image, seed, segments: bool):
    h, w = image.shape[:2]
    rng = np.random.RandomState(seed)
    if segments:
        _, mask, joints = pkg.keypoints.raw_sample(np.zeros((h, w, 3), np.uint8), annotation(h, w, seed))
    else:
        mask = rng.rand(h, w) < 0.2
        joints = np.concatenate([rng.uniform(0, [w, h], (2, 17, 2)), rng.randint(0, 3, (2, 17, 1))], -1)
    return image, mask, joints


def test_train_input_takes_jpeg_images(J, pkg):
    ti_mod = pkg.keypoints.train_input
    S = 64
    ti = ti_mod.TrainInput(S, [1 / 4, 1 / 2], device=DEV)
    use = ["420_120x200_scene_q90_plain", "420_120x200_scene_q90_rows1", "420_33x50_scene_q90_plain", "420_36x44_noise_q90_plain", "422_21x43_scene_q90_plain",
           "444_17x23_scene_q90_plain", "420_130x24_noise_q90_rows1"]
    arrays = {n: corpus()[n][1] for n in use}
    jpegs = {n: J.JpegImage(corpus()[n][0]) for n in use}
    extra = picture("scene", 40, 48)  # a sample that is an array in both batches

    def batch(images):
        tiles = [_sample(pkg, images[n], 10 + i, False) for i, n in enumerate(use[2:6])]
        return [_sample(pkg, images[use[0]], 1, True), _sample(pkg, extra, 2, False), ti_mod.Mosaic(tiles), _sample(pkg, images[use[1]], 3, False),
                _sample(pkg, images[use[6]], 4, False)]

    param = lambda h, w, i: ti_mod.AugParams(min(h, w) / 200 * (0.8 + 0.2 * i), 25.0 * i - 30, (w / 2 + 3 * i, h / 2 - 2 * i), bool(i % 2))  # noqa: E731
    params = [param(120, 200, 0), param(40, 48, 1), param(2 * S, 2 * S, 2), param(120, 200, 3), param(130, 24, 4)]
    want = ti.build(batch(arrays), params)
    array_bytes, array_staged, array_launches = ti.last_h2d_bytes, ti.last_staged_bytes, ti.last_launches
    assert ti.jpeg_status().size == 0
    got = ti.build(batch(jpegs), params)
    assert_same_batch(got, want)
    assert ti.jpeg_status().tolist() == [0] * 7
    assert ti.last_launches == array_launches + 3
    # the staged copy: the array sample's pixels and the dense masks, rounded up to 64 | 5 hh_train_desc | 1 hh_mosaic_desc | the crowd
    # tables of the one segment sample, rounded up to 16 | 7 hh_jpeg_dec_desc | every stream and table block, each rounded up to 16
    seg = batch(jpegs)[0][1]
    dense_masks = sum(arrays[n].shape[0] * arrays[n].shape[1] for n in use[1:])
    plain = (extra.size + extra.shape[0] * extra.shape[1] + dense_masks + 63) // 64 * 64 + 272 * 5 + 112 + seg.table_bytes
    staged = (plain + 15) // 16 * 16 + 64 * 7 + sum(j.staged_bytes() for j in jpegs.values())
    assert all(j.staged_bytes() == (j.data.size + 15) // 16 * 16 + (112 + 7808 + 32 * len(j.segments) + 15) // 16 * 16 for j in jpegs.values())
    assert ti.last_staged_bytes == staged
    assert ti.last_h2d_bytes - staged == array_bytes - array_staged  # (the joint tables, the same in both)
    # the scene entries alone: fewer bytes cross than for their pixels
    scene = [n for n in use if "scene" in n and "120x200" in n]
    ti.build([_sample(pkg, arrays[n], 5, False) for n in scene], params[:1] * 2)
    scene_array_bytes = ti.last_h2d_bytes
    ti.build([_sample(pkg, jpegs[n], 5, False) for n in scene], params[:1] * 2)
    assert ti.last_h2d_bytes < scene_array_bytes
    ti.jpeg_status()
    # a batch without a JpegImage is what it was: same bytes, same launches
    assert_same_batch(ti.build(batch(arrays), params), want)
    assert (ti.last_h2d_bytes, ti.last_launches) == (array_bytes, array_launches)


def test_mjpeg_reader_reads_what_the_writer_wrote(J, tmp_path):
    frames = [J.encode_jpeg_host(np.roll(picture("scene", 40, 56), 5 * i, axis=1), 90, 420 if i % 2 else 444) for i in range(4)]
    with J.MJPEGWriter(tmp_path / "clip.avi", 30, 56, 40) as wr:
        for f in frames:
            wr.write(f)
    rd = J.MJPEGReader(tmp_path / "clip.avi")
    assert len(rd) == 4 and rd.fps == 30
    got = rd.read(1, 3, DEV)
    assert len(got) == 3
    for g, f in zip(got, frames[1:]):
        assert np.array_equal(g.cpu().numpy(), J.decode_jpeg_host(f))
    assert np.array_equal(rd.read(0, 1, DEV, bgr=True)[0].cpu().numpy(), J.decode_jpeg_host(frames[0], bgr=True))
