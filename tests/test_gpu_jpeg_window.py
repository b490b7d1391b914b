"""hh_jpeg_decode_window_u8_batch on the GPU against the same code compiled for the host (hh_debug_jpeg_decode_window_host; its
parity with Pillow's pixels over a window lattice is tests/test_jpeg_window_cpu.py) and against the slice of Pillow's pixels of
tests/golden/jpeg_decode.npz: one batched call over all four samplings, restart and indexed streams and mixed windows, with guard
bands and pitched rows; decode_jpeg_device(windows=...); JpegImage samples in ClsInput and InferenceClassificationModel, bit for bit
against the array samples; the status path on a truncated stream.  Tiny images only; Pillow is not imported here."""
import importlib

import numpy as np
import pytest
import torch

from conftest import PKG
from test_jpeg_decode_cpu import corpus, names, truncated_stream

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (corpus entry, mcus per segment of its index or None for the stream's own segments, window or None for the whole image)
BATCH = [("420_120x200_scene_q90_plain", None, (40, 70, 30, 40)),   # an index built on the spot (one MCU row)
         ("420_120x200_scene_q90_rows1", None, (0, 0, 120, 200)),    # restart segments, the whole image as a window
         ("420_33x50_noise_q75_plain", 1, (15, 15, 2, 18)),          # one MCU per segment: the selected set is not contiguous
         ("422_21x43_noise_q90_plain", 2, (7, 16, 9, 16)),           # h2v1: left at an MCU edge, the last column one before the next
         ("444_17x23_noise_q30_plain", 1, (8, 7, 9, 16)),            # touches the bottom and right edge of an odd-sized image
         ("400_17x23_scene_q90_plain", None, (16, 0, 1, 23)),        # grayscale, one pixel high
         ("420_130x24_scene_q90_own", None, (3, 23, 127, 1)),        # this project's encoder, RSTm wraps past 7; one pixel wide
         ("420_16x4_scene_q90_plain", None, (1, 1, 14, 3)),          # chroma width 2: the replication rule
         ("420_1x1_scene_q90_plain", None, (0, 0, 1, 1)),
         ("420_36x44_noise_q90_plain", 2, (17, 3, 6, 11))]           # a small window inside one MCU; two MCUs per segment


@pytest.fixture(scope="module")
def J(pkg):
    return importlib.import_module(PKG + ".keypoints.jpeg")


@pytest.fixture(scope="module")
def batch(J):
    """The batch's JpegImage items, windows, host-twin pixels (computed once, left unchanged)."""
    items, wins, want = [], [], []
    for name, mps, win in BATCH:
        data, pixels = corpus()[name]
        index = None if mps is None else J.build_jpeg_index(data, mps)
        items.append(J.JpegImage(data, index))
        wins.append(win)
        t, l, hh, ww = win
        host = J.decode_jpeg_host(data, index=items[-1].segments, window=win)
        assert np.array_equal(host, pixels[t:t + hh, l:l + ww]), name  # so what equals the host twin equals Pillow
        host.setflags(write=False)
        want.append(host)
    return items, wins, want


def test_one_batched_call_equals_the_host_twin_and_keeps_its_guard_bands(J, batch):
    items, wins, want = batch
    gap, extra = 256, 7  # bytes between destinations; pixels beyond `width` in every pitched row
    sizes = [hh * (ww + extra) * 3 for _, _, hh, ww in wins]
    offs = np.cumsum([gap] + [(s + gap + 15) // 16 * 16 for s in sizes])
    slab = torch.full((int(offs[-1]),), 0xA5, dtype=torch.uint8, device=DEV)
    wide = [slab[int(o):int(o) + s].view(hh, ww + extra, 3) for o, s, (_, _, hh, ww) in zip(offs, sizes, wins)]
    out = [v[:, :ww] for v, (_, _, _, ww) in zip(wide, wins)]
    got = J.decode_jpeg_device(items, device=DEV, out=out, windows=wins)
    assert J.decode_jpeg_device.last_status.tolist() == [0] * len(items)
    host = slab.cpu().numpy()
    for j, (o, s, (_, _, hh, ww)) in enumerate(zip(offs, sizes, wins)):
        rows = host[int(o):int(o) + s].reshape(hh, ww + extra, 3)
        assert got[j].data_ptr() == out[j].data_ptr()
        assert np.array_equal(rows[:, :ww], want[j]), BATCH[j][0]
        assert bool((rows[:, ww:] == 0xA5).all()), BATCH[j][0]                      # beyond 3 * width in the pitched rows
        assert bool((host[int(o) - gap:int(o)] == 0xA5).all()) and bool((host[int(o) + s:int(o) + s + gap] == 0xA5).all()), BATCH[j][0]
    # what crossed: the descriptors, then per image the slice and the table block of the selected segments, each rounded up to 16
    plans = [it.window_plan(w) for it, w in zip(items, wins)]
    assert J.decode_jpeg_device.last_h2d_bytes == 80 * len(items) + sum(p.staged_bytes for p in plans)
    assert plans[0].slice[1] - plans[0].slice[0] < items[0].data.size and plans[0].nsel == 3 < len(items[0].segments)


def test_decode_jpeg_device_with_windows_and_with_whole_images_mixed_in(J, batch):
    items, wins, want = batch
    got = J.decode_jpeg_device(items, device=DEV, windows=wins)
    for j, g in enumerate(got):
        assert g.dtype == torch.uint8 and tuple(g.shape) == want[j].shape and g.is_contiguous(), BATCH[j][0]
        assert np.array_equal(g.cpu().numpy(), want[j]), BATCH[j][0]
    # bytes in place of JpegImage, B,G,R for some, every second window None: those come back whole
    streams = [corpus()[name][0] for name, _, _ in BATCH]
    mixed = [None if j % 2 else w for j, w in enumerate(wins)]
    bgr = [j % 3 == 0 for j in range(len(BATCH))]
    got = J.decode_jpeg_device(streams, bgr=bgr, device=DEV, windows=mixed)
    for j, g in enumerate(got):
        ref = corpus()[BATCH[j][0]][1] if mixed[j] is None else want[j]
        assert np.array_equal(g.cpu().numpy(), ref[:, :, ::-1] if bgr[j] else ref), BATCH[j][0]
    # without a window the function is what it was
    whole = J.decode_jpeg_device(streams[:3], device=DEV, windows=[None] * 3)
    for g, (name, _, _) in zip(whole, BATCH):
        assert np.array_equal(g.cpu().numpy(), corpus()[name][1])
    with pytest.raises(ValueError, match="one entry per stream"):
        J.decode_jpeg_device(streams[:3], device=DEV, windows=[None] * 2)


def test_the_whole_image_entry_is_the_window_entry_with_every_window_the_whole_image(J, pkg):
    """One batch through hh_jpeg_decode_u8_batch and through hh_jpeg_decode_window_u8_batch with the windows (0, 0, h, w): every
    sampling, restart segments, a 2-MCU index, the smallest stream of the corpus (one MCU) and a truncated stream, which ends in its
    status in both calls (the destinations are given, so the pixels are there although the call raises)."""
    cut, cut_index = truncated_stream(J)
    smallest = min(names(), key=lambda n: (corpus()[n][1].size, len(corpus()[n][0])))  # the fewest pixels (1 x 1), then the fewest bytes
    picks = [("444_17x23_noise_q30_plain", None), ("422_21x43_noise_q90_plain", 2), ("420_120x200_scene_q90_rows1", None),
             ("400_17x23_scene_q90_plain", None), (smallest, None)]
    items = [J.JpegImage(corpus()[n][0], None if mps is None else J.build_jpeg_index(corpus()[n][0], mps)) for n, mps in picks]
    items.append(J.JpegImage(cut, cut_index))
    infos = [J.jpeg_info(it.data) for it in items]
    assert {i.sampling for i in infos} == {444, 422, 420, 400} and infos[2].restart_interval and infos[4].mcu_cols * infos[4].mcu_rows == 1
    runs = []
    for windows in (None, [(0, 0, it.h, it.w) for it in items]):
        out = [torch.full(it.shape, 0xA5, dtype=torch.uint8, device=DEV) for it in items]
        with pytest.raises(pkg._lib.HHError, match=r"image 5: status 3 \(bytes exhausted\)"):
            J.decode_jpeg_device(items, device=DEV, out=out, windows=windows)
        runs.append((J.decode_jpeg_device.last_status.tolist(), [o.cpu().numpy() for o in out], J.decode_jpeg_device.last_h2d_bytes))
    (status_a, pixels_a, bytes_a), (status_b, pixels_b, bytes_b) = runs
    assert status_a == status_b == [0, 0, 0, 0, 0, 3]
    for j, (name, _) in enumerate(picks):
        assert np.array_equal(pixels_a[j], pixels_b[j]) and np.array_equal(pixels_a[j], corpus()[name][1]), name
    # which entry ran: 64-byte descriptors and whole streams against 80-byte descriptors and the windows' slices
    assert bytes_a == 64 * 6 + sum(it.staged_bytes() for it in items)
    assert bytes_b == 80 * 6 + sum(it.window_plan((0, 0, it.h, it.w)).staged_bytes for it in items) < bytes_a


def test_load_jpeg_with_a_window(J, tmp_path):
    data, pixels = corpus()["420_33x50_scene_q90_plain"]
    path = tmp_path / "a.jpg"
    path.write_bytes(data)
    cache = J.JpegIndexCache()
    assert np.array_equal(J.load_jpeg(path, DEV, cache, window=(9, 11, 20, 30)).cpu().numpy(), pixels[9:29, 11:41])
    assert np.array_equal(J.load_jpeg(path, DEV, cache, bgr=True, window=(0, 49, 33, 1)).cpu().numpy(), pixels[:, 49:, ::-1])


CLS = ["420_120x200_scene_q90_plain", "420_120x200_scene_q90_rows1", "422_21x43_scene_q90_plain", "444_17x23_scene_q90_plain", "400_17x23_scene_q90_plain",
       "420_33x50_noise_q75_plain"]


def _cls_params(inp, S):
    return [inp.CropParams(40, 70, 30, 40, True), inp.inference_geometry(120, 200, resize=S + 4, crop=S), inp.CropWindow(3, 16, 17, 20, S + 3, S + 5, 2, 1, True, False),
            inp.CropParams(0, 0, 17, 23), inp.CropParams(16, 22, 1, 1, True), inp.CropWindow(15, 15, 18, 33, 2 * S, S, S // 2, 0)]


def test_cls_input_builds_the_same_batch_from_jpeg_images_as_from_their_pixels(J, pkg):
    inp = importlib.import_module(PKG + ".classification.input")
    S = 16
    ci = inp.ClsInput(S, device=DEV)
    arrays = [(np.ascontiguousarray(corpus()[n][1]), 10 + i) for i, n in enumerate(CLS)]
    jpegs = [(J.JpegImage(corpus()[n][0]), 10 + i) for i, n in enumerate(CLS)]
    params = _cls_params(inp, S)
    want_images, want_targets = ci.build(arrays, params)
    array_bytes = ci.last_h2d_bytes
    assert ci.last_launches == 1 and ci.jpeg_status().size == 0
    got_images, got_targets = ci.build(jpegs, params)
    assert torch.equal(got_images, want_images) and torch.equal(got_targets, want_targets)  # bit for bit: the same launch reads identical bytes
    assert ci.last_launches == 4 and ci.jpeg_status().tolist() == [0] * 6
    # a batch mixing both kinds
    mixed = [jpegs[b] if b % 2 else arrays[b] for b in range(len(CLS))]
    got_images, got_targets = ci.build(mixed, params)
    assert torch.equal(got_images, want_images) and torch.equal(got_targets, want_targets)
    assert ci.last_launches == 4 and ci.jpeg_status().tolist() == [0] * 3
    # what crossed for the all-JPEG batch: no pixels; 6 crop descriptors and targets behind a 64-aligned (empty) pixel area; 6 window
    # descriptors; the staged slices and table blocks
    plans = [j.window_plan((q.top, q.left, q.height, q.width)) for (j, _), q in
             zip(jpegs, (ci.window(j.h, j.w, p) for (j, _), p in zip(jpegs, params)))]
    ci.build(jpegs, params)
    assert ci.last_h2d_bytes == (56 * 6 + 8 * 6 + 15) // 16 * 16 + 80 * 6 + sum(p.staged_bytes for p in plans)
    # an array batch is what it was: same bytes, one launch
    again, _ = ci.build(arrays, params)
    assert torch.equal(again, want_images) and (ci.last_h2d_bytes, ci.last_launches) == (array_bytes, 1)


def test_cls_input_ships_fewer_bytes_where_that_is_arithmetically_certain(J, pkg):
    """The whole 120 x 200 image as the source rectangle (the inference form): the array sample ships 120 * 200 * 3 = 72000 pixel bytes;
    the JpegImage ships at most its whole file (rounded up to 16), a table block of 112 + 7808 + 32 * 8 bytes for its 8 MCU rows and an
    80-byte descriptor more, and the file is below 32 KiB: under 41 KiB in all."""
    inp = importlib.import_module(PKG + ".classification.input")
    data, pixels = corpus()["420_120x200_scene_q90_plain"]
    item = J.JpegImage(data)
    assert len(data) < 32768 and len(item.segments) == 8
    ci = inp.ClsInput(16, device=DEV)
    geometry = [inp.inference_geometry(120, 200, resize=18, crop=16)]
    want, _ = ci.build([(np.ascontiguousarray(pixels), 1)], geometry)
    array_bytes = ci.last_h2d_bytes
    got, _ = ci.build([(item, 1)], geometry)
    assert torch.equal(got, want) and ci.jpeg_status().tolist() == [0]
    assert array_bytes >= 72000 and ci.last_h2d_bytes < 32768 + 16 + 8192 + 80 + 128 < array_bytes


def test_inference_model_takes_jpeg_images_and_bytes(J, pkg):
    cls = importlib.import_module(PKG + ".classification")
    net = pkg.ClassificationHRNet(32, 1000)
    net.load_state_dict({k: torch.from_numpy(pkg.synth.synth_param(k, v.shape, 3)) for k, v in net.state_dict().items()})
    model = cls.InferenceClassificationModel(net, {i: i for i in range(1000)}, input_size=64, device=DEV)
    use = CLS[:3]
    arrays = [np.ascontiguousarray(corpus()[n][1]) for n in use]
    compressed = [J.JpegImage(corpus()[use[0]][0]), corpus()[use[1]][0], arrays[2]]  # a JpegImage, raw bytes, and an array in one batch
    assert torch.equal(model.prepare_inputs(compressed), model.prepare_inputs(arrays))
    want = model.infer_images(arrays)
    got = model.infer_images(compressed)
    for g, w in zip(got, want):
        assert np.array_equal(g.logits, w.logits) and g.prediction == w.prediction
    single = model(corpus()[use[0]][0])
    assert np.array_equal(single.logits, model(arrays[0]).logits)
    progressive_like = b"\xff\xd8\xff\xc2\x00\x11\x08" + bytes(20)  # SOI, then an SOF2 frame header
    with pytest.raises(pkg._lib.HHError, match="progressive"):
        model.prepare_inputs([progressive_like])


def test_a_truncated_stream_raises_its_status_and_leaves_the_other_images_alone(J, pkg):
    """The malformed-input status path (as tests/test_gpu_jpeg_decode.py has it for the whole decode): a stream cut 10 bytes before its
    EOI, with the index of the whole stream.  Only the last MCU row's segment runs dry."""
    inp = importlib.import_module(PKG + ".classification.input")
    cut, cut_index = truncated_stream(J)
    S = 16
    ci = inp.ClsInput(S, device=DEV)
    clean = [(J.JpegImage(corpus()[n][0]), i) for i, n in enumerate(CLS[:3])]
    params = _cls_params(inp, S)[:3]
    want, _ = ci.build(clean, params)
    samples = [clean[0], (J.JpegImage(cut, cut_index), 7), clean[1], clean[2]]
    # rows 20..32, columns 5..49: MCU rows 1..2 up to the last MCU column, where the cut lies
    got, _ = ci.build(samples, [params[0], inp.CropParams(20, 5, 13, 45), params[1], params[2]])
    assert ci.jpeg_status(check=False).tolist() == [0, 3, 0, 0]
    with pytest.raises(pkg._lib.HHError, match=r"image 1: status 3 \(bytes exhausted\)"):
        ci.jpeg_status()
    assert torch.equal(got[[0, 2, 3]], want)
    # the same stream, windows the cut lies behind (MCU row 0; MCU rows 1..2 without the last MCU column): nothing is wrong with what
    # is walked
    whole = corpus()["420_33x50_noise_q75_plain"][1]
    got = J.decode_jpeg_device([J.JpegImage(cut, cut_index)], device=DEV, windows=[(20, 5, 13, 40)])[0]
    assert np.array_equal(got.cpu().numpy(), whole[20:33, 5:45])
    got = J.decode_jpeg_device([J.JpegImage(cut, cut_index)], device=DEV, windows=[(0, 0, 8, 50)])[0]
    assert np.array_equal(got.cpu().numpy(), whole[:8])
    with pytest.raises(pkg._lib.HHError, match=r"image 0: status 3 \(bytes exhausted\)"):
        J.decode_jpeg_device([J.JpegImage(cut, cut_index)], device=DEV, windows=[(0, 0, 33, 50)])
