"""The window decode's rule on the host (no GPU): hh_debug_jpeg_decode_window_host == the slice of Pillow's pixels of
tests/golden/jpeg_decode.npz, byte for byte, for every corpus stream and every window of a fixed lattice; with B,G,R, a pitched
destination, indexes of one MCU row, 2 MCUs and 1 MCU per segment, and the restart segments; the counts struct against values derived
here from the header's rule; every refusal by name before anything is written; truncation inside and after the walked part; ClsInput's
geometry for a JpegImage."""
import ctypes as C
import functools
import importlib
import re

import numpy as np
import pytest
import torch

from conftest import PKG
from test_jpeg_decode_cpu import bad_code_stream, corpus, names, truncated_stream


@pytest.fixture(scope="module")
def J(pkg):
    return importlib.import_module(PKG + ".keypoints.jpeg")


FACTORS = {444: (1, 1), 422: (2, 1), 420: (2, 2), 400: (1, 1)}


def lattice(h: int, w: int, hs: int, vs: int) -> list:
    """The windows (top, left, height, width) of one image, so far as its size allows them (each is cut to the image; duplicates go)."""
    Mh, Mw = 8 * vs, 8 * hs
    want = [(0, 0, h, w),                                                          # the whole image
            (0, 0, 1, 1), (0, w - 1, 1, 1), (h - 1, 0, 1, 1), (h - 1, w - 1, 1, 1), (h // 2, w // 2, 1, 1),  # 1 x 1: corners, middle
            (Mh, Mw, h, w), (Mh, Mw, 3, 3), (2 * Mh, 0, 5, w), (0, 2 * Mw, h, 5),    # top / left a multiple of the MCU: neighbour in the previous MCU
            (0, 0, Mh, Mw), (1, 1, Mh - 1, Mw - 1), (3, 3, 2 * Mh - 3, 2 * Mw - 3),  # last row / column one before a multiple: neighbour in the next MCU
            (h - 3, w - 3, 3, 3), (h - Mh - 1, w - Mw - 1, h, w), (0, w - 2, h, 2), (h - 2, 0, 2, w),  # touching the right and bottom edge
            (Mh + 2, Mw + 2, 3, 3), (2, 2, 3, 3),                                  # entirely inside one MCU
            (0, 0, 1, w), (h // 2, 0, 1, w), (h - 1, 0, 1, w), (Mh - 1, 0, 1, w), (Mh, 0, 1, w),  # one pixel high, full width
            (0, 0, h, 1), (0, w // 2, h, 1), (0, w - 1, h, 1), (0, Mw - 1, h, 1), (0, Mw, h, 1)]  # one pixel wide, full height
    out = []
    for t, l, hh, ww in want:
        t, l = min(max(t, 0), h - 1), min(max(l, 0), w - 1)
        win = (t, l, max(1, min(hh, h - t)), max(1, min(ww, w - l)))
        if win not in out:
            out.append(win)
    return out


def rectangle(info, win) -> tuple:
    """The MCU rectangle of a window, from the header's rule -> (mx0, mx1, my0, my1), inclusive."""
    hs, vs = FACTORS[info.sampling]
    t, l, hh, ww = win
    b, r = t + hh - 1, l + ww - 1
    rows, cols = [t // (8 * vs), b // (8 * vs)], [l // (8 * hs), r // (8 * hs)]
    if info.components == 3 and vs == 2:
        ch = (info.h + 1) // 2
        rows += [max(0, (t >> 1) - 1) // 8, min(ch - 1, (b >> 1) + 1) // 8]
    if info.components == 3 and hs == 2:
        cw = (info.w + 1) // 2
        cols += [max(0, (l >> 1) - 1) // 8, min(cw - 1, (r >> 1) + 1) // 8]
    return min(cols), max(cols), min(rows), max(rows)


def expected_counts(info, segments, win) -> dict:
    """What a window decode does, derived from the rule by brute force over the MCUs of every segment."""
    mx0, mx1, my0, my1 = rectangle(info, win)
    bpm = 1 if info.components == 1 else FACTORS[info.sampling][0] * FACTORS[info.sampling][1] + 2
    walked_segments = walked = 0
    lo, hi = None, None
    for s in segments:
        first, count = int(s["first_mcu"]), int(s["mcu_count"])
        inside = [m for m in range(first, first + count) if mx0 <= m % info.mcu_cols <= mx1 and my0 <= m // info.mcu_cols <= my1]
        if not inside:
            continue
        walked_segments += 1
        walked += inside[-1] - first + 1
        end = min(int(s["byte_end"]) >> 1, info.scan_end)
        lo = int(s["byte_offset"]) if lo is None else min(lo, int(s["byte_offset"]))
        hi = end if hi is None else max(hi, end)
    stored = (mx1 - mx0 + 1) * (my1 - my0 + 1)
    return dict(segments_walked=walked_segments, mcus_walked=walked, mcus_stored=stored, blocks_transformed=stored * bpm, pixels_written=win[2] * win[3],
                stream_bytes=hi - lo)


@functools.lru_cache(maxsize=None)
def indexes(name: str) -> dict:
    """The segment sets one stream is decoded through: its own (None: restart segments, or the whole scan as one segment), and indexes
    of one MCU row, 2 MCUs and 1 MCU per segment."""
    J = importlib.import_module(PKG + ".keypoints.jpeg")
    data = corpus()[name][0]
    return {"own": None, "row": J.build_jpeg_index(data), "2": J.build_jpeg_index(data, 2), "1": J.build_jpeg_index(data, 1)}


def own_segments(J, data) -> np.ndarray:
    """What the host twin decodes through when no index is given."""
    info = J.jpeg_info(data)
    if info.restart_interval:
        return J.JpegImage(data).segments
    seg = np.zeros(1, J.SEGMENT)
    seg[0] = (0, info.mcu_cols * info.mcu_rows, info.scan_offset, 0, (0, 0, 0), info.scan_end << 1)
    return seg


@pytest.mark.parametrize("name", names())
def test_every_window_equals_the_golden_slice_and_the_counts_are_the_rules(J, name):
    data, pixels = corpus()[name]
    info = J.jpeg_info(data)
    hs, vs = FACTORS[info.sampling]
    for win in lattice(info.h, info.w, hs, vs):
        t, l, hh, ww = win
        want = pixels[t:t + hh, l:l + ww]
        for key, index in indexes(name).items():
            counts = {}
            got = J.decode_jpeg_host(data, index=index, window=win, counts=counts)
            assert got.shape == want.shape and np.array_equal(got, want), (name, win, key, np.argwhere(got != want)[:4])
            assert counts == expected_counts(info, own_segments(J, data) if index is None else index, win), (name, win, key)
            if key == "row" and not info.restart_interval:  # the closed form of the one-MCU-row index
                mx0, mx1, my0, my1 = rectangle(info, win)
                assert counts["segments_walked"] == my1 - my0 + 1 and counts["mcus_walked"] == (my1 - my0 + 1) * (mx1 + 1)
        # B,G,R, and a pitch above 3 * width (through the index of one MCU per segment)
        assert np.array_equal(J.decode_jpeg_host(data, bgr=True, window=win), want[:, :, ::-1]), (name, win)
        assert np.array_equal(J.decode_jpeg_host(data, index=indexes(name)["1"], window=win, pitch=3 * ww + 5), want), (name, win)


def test_the_corpus_has_restart_streams_and_the_lattice_its_cases(J):
    restart = [n for n in names() if J.jpeg_info(corpus()[n][0]).restart_interval]
    assert restart and any("own" in n for n in restart)
    narrow = [n for n in names() if J.jpeg_info(corpus()[n][0]).w <= 4 and J.jpeg_info(corpus()[n][0]).sampling in (420, 422)]
    assert narrow  # the replication rule
    wins = lattice(33, 50, 2, 2)
    assert (0, 0, 33, 50) in wins and (16, 16, 17, 34) in wins and (1, 1, 15, 15) in wins and (30, 47, 3, 3) in wins and (18, 18, 3, 3) in wins
    assert (15, 0, 1, 50) in wins and (0, 16, 33, 1) in wins


def test_a_small_window_does_strictly_less_than_the_whole_image(J):
    data, pixels = corpus()["420_120x200_scene_q90_plain"]
    index = J.build_jpeg_index(data)
    whole, part = {}, {}
    J.decode_jpeg_host(data, index=index, window=(0, 0, 120, 200), counts=whole)
    got = J.decode_jpeg_host(data, index=index, window=(40, 70, 30, 40), counts=part)
    assert np.array_equal(got, pixels[40:70, 70:110])
    # rows 40..69 need chroma rows 19..35: MCU rows 2..4; columns 70..109 need chroma columns 34..55: MCU columns 4..6
    assert part == dict(segments_walked=3, mcus_walked=3 * 7, mcus_stored=9, blocks_transformed=54, pixels_written=1200, stream_bytes=part["stream_bytes"])
    assert whole["segments_walked"] == 8 and whole["mcus_walked"] == whole["mcus_stored"] == 8 * 13
    assert all(part[k] < whole[k] for k in whole), (part, whole)
    info = J.jpeg_info(data)
    assert whole["stream_bytes"] == info.scan_end - info.scan_offset
    # a whole-image window gives the bytes of the whole decode
    assert np.array_equal(J.decode_jpeg_host(data, window=(0, 0, 120, 200)), J.decode_jpeg_host(data))


def test_the_whole_image_is_the_window_that_covers_it(J, pkg):
    """What the one decoder rests on: hh_debug_jpeg_decode_host and hh_debug_jpeg_decode_window_host with the window (0, 0, h, w) give
    the same bytes through every segment set, the window's rectangle is the MCU grid, and a malformed scan ends in the same status."""
    for name in names():
        data = corpus()[name][0]
        info = J.jpeg_info(data)
        nmcu = info.mcu_cols * info.mcu_rows
        bpm = 1 if info.components == 1 else FACTORS[info.sampling][0] * FACTORS[info.sampling][1] + 2
        for key, index in indexes(name).items():
            counts = {}
            got = J.decode_jpeg_host(data, index=index, window=(0, 0, info.h, info.w), counts=counts)
            assert np.array_equal(got, J.decode_jpeg_host(data, index=index)), (name, key)
            assert counts["mcus_walked"] == counts["mcus_stored"] == nmcu and counts["blocks_transformed"] == nmcu * bpm, (name, key, counts)
            assert counts["pixels_written"] == info.h * info.w, (name, key, counts)

    def status(stream, index, window):
        with pytest.raises(pkg._lib.HHError, match=r"status \d") as e:
            J.decode_jpeg_host(stream, index=index, window=window)
        return int(re.search(r"status (\d)", str(e.value)).group(1))

    cut, index = truncated_stream(J)
    bad, _ = bad_code_stream(J, pkg)
    for stream, index, want in ((cut, index, 3), (bad, None, 1)):
        info = J.jpeg_info(stream)
        assert status(stream, index, None) == status(stream, index, (0, 0, info.h, info.w)) == want


def test_window_plan_reports_the_selected_segments_and_the_slice(J):
    data, _ = corpus()["420_120x200_scene_q90_plain"]
    item = J.JpegImage(data, J.build_jpeg_index(data, 2))
    plan = item.window_plan((40, 70, 30, 40))
    want = expected_counts(J.jpeg_info(data), item.segments, (40, 70, 30, 40))
    assert plan.nsel == want["segments_walked"] == 6 and plan.slice[1] - plan.slice[0] == want["stream_bytes"]  # 3 rows x MCUs 4..6: two pairs each
    assert plan.tables_bytes == 112 + 7808 + 32 * plan.nsel
    assert plan.staged_bytes == (want["stream_bytes"] + 15) // 16 * 16 + (plan.tables_bytes + 15) // 16 * 16
    assert plan.ws_bytes == 9 * 6 * 128 + 48 * 48 + 2 * 24 * 24  # coefficients of 9 MCUs, a 48 x 48 luma plane, two 24 x 24 chroma planes
    stage = np.full(plan.staged_bytes + 32, 0xA5, np.uint8)
    stream_at, tables_at, _, info = item.stage_window(stage, 16, (40, 70, 30, 40))
    assert stream_at == 16 and tables_at == 16 + (want["stream_bytes"] + 15) // 16 * 16
    assert bytes(stage[16:16 + want["stream_bytes"]]) == data[plan.slice[0]:plan.slice[1]]
    assert int(info[0]["scan_offset"]) == 0 and int(info[0]["scan_end"]) == want["stream_bytes"]
    segs = stage[tables_at + 112 + 7808:tables_at + plan.tables_bytes].view(J.SEGMENT)
    assert int(segs["byte_offset"].min()) == 0 and int((segs["byte_end"] >> 1).max()) == want["stream_bytes"]
    assert bool((stage[:16] == 0xA5).all()) and bool((stage[tables_at + plan.tables_bytes:] == 0xA5).all())


def _host_call(J, pkg, data, win, pitch=None, entries=None, flags=0):
    lib = pkg._lib.load()
    a = np.frombuffer(data, np.uint8)
    w = np.zeros(1, J.WINDOW)
    w[0] = win
    dst = np.full(64 * 64 * 3, 0xA5, np.uint8)
    status = C.c_int(-7)
    rc = lib.hh_debug_jpeg_decode_window_host(a.ctypes.data, a.size, None if entries is None else entries.ctypes.data, 0 if entries is None else len(entries),
                                              w.ctypes.data, flags, dst.ctypes.data, 3 * win[3] if pitch is None else pitch, C.byref(status), None)
    return rc, dst, lib.hh_last_error().decode()


def test_the_host_twin_refuses_by_name_before_anything_is_written(J, pkg):
    data, _ = corpus()["420_33x50_scene_q90_plain"]
    index = J.build_jpeg_index(data, 1)
    for kwargs, message in ((dict(win=(0, 0, 0, 5)), "the window is empty"), (dict(win=(0, 0, 5, 0)), "the window is empty"),
                            (dict(win=(30, 0, 4, 5)), "the window leaves the image"), (dict(win=(0, 46, 4, 5)), "the window leaves the image"),
                            (dict(win=(-1, 0, 4, 5)), "the window leaves the image"), (dict(win=(0, 0, 4, 5), pitch=14), "pitch below 3 \\* width"),
                            (dict(win=(0, 0, 4, 5), flags=2), "unknown flag"),
                            # an index that lacks the window's MCUs: the selected set is empty
                            (dict(win=(20, 20, 4, 5), entries=index[:2].copy()), "no segment holds an MCU of the window's rectangle")):
        rc, dst, err = _host_call(J, pkg, data, **kwargs)
        assert rc == 1 and bool((dst == 0xA5).all()), kwargs
        assert re.search(message, err), (kwargs, err)
    rc, dst, _ = _host_call(J, pkg, data, (0, 0, 4, 5))
    assert rc == 0 and bool((dst[60:] == 0xA5).all()) and not bool((dst[:60] == 0xA5).all())
    with pytest.raises(pkg._lib.HHError, match="the window leaves the image"):
        J.JpegImage(data).window_plan((0, 0, 34, 50))
    with pytest.raises(pkg._lib.HHError, match="the window is empty"):
        J.decode_jpeg_host(data, window=(0, 0, 0, 0))


def test_the_batch_entry_refuses_by_name_before_any_launch(J, pkg):
    """Every check is made on the HOST copies before the first use of a device pointer: the device addresses here are made up and are
    never dereferenced (no GPU is needed, and none is touched)."""
    lib = pkg._lib.load()
    data, _ = corpus()["420_33x50_scene_q90_plain"]
    item = J.JpegImage(data)
    win = (5, 7, 20, 30)
    plan = item.window_plan(win)
    stage = np.zeros(plan.staged_bytes, np.uint8)
    stream_at, tables_at, _, info = item.stage_window(stage, 0, win, plan)
    base = 1 << 20  # a made-up, 16-byte aligned device address

    def call(n=1, descs_dev=base + 4096, work=base + 8192, status=base + 16384, ws_bytes=plan.ws_bytes, info=info, **fields):
        desc = np.zeros(1, J.WIN_DESC)
        desc[0] = item.window_desc(plan, stream_at, 1024 + tables_at, 65536, 0, 3 * win[3])
        for k, v in fields.items():
            (desc["d"] if k in J.DEC_DESC.names else desc)[k][0] = v  # (hh_jpeg_win_desc: the decode descriptor `d`, then the window)
        return lib.hh_jpeg_decode_window_u8_batch(base, descs_dev, desc.ctypes.data, info.ctypes.data, n, work, ws_bytes, status, None), lib.hh_last_error().decode()

    wrong = info.copy()
    wrong["mcols"] += 1
    for kwargs, message in ((dict(window=(0, 0, 0, 30)), "the window is empty"), (dict(window=(14, 7, 20, 30)), "the window leaves the image"),
                            (dict(window=(5, 21, 20, 30)), "the window leaves the image"), (dict(pitch=89), "pitch below 3 * width"),
                            (dict(ws_bytes=plan.ws_bytes - 1), "workspace below hh_jpeg_decode_window_workspace_bytes"),
                            (dict(tables_bytes=plan.tables_bytes - 1), "table block below hh_jpeg_decode_tables_bytes"),
                            (dict(nseg=0), "no selected segment"), (dict(descs_dev=base + 4100), "descs_dev must be 8-byte"),
                            (dict(work=base + 8200), "workspace 16-byte"), (dict(status=base + 16386), "status_dev 4-byte"),
                            (dict(tables_offset=1024 + tables_at + 8), "16-byte aligned"), (dict(ws_offset=8), "16-byte aligned"),
                            (dict(dst_offset=-1), "negative offset"), (dict(n=0), "need 1 <= n"), (dict(flags=2), "unknown flag"),
                            (dict(info=wrong), "bad stream info"), (dict(stream_length=plan.slice[1] - plan.slice[0] - 1), "outside the slice's length"),
                            (dict(descs_dev=None), "null pointer")):
        rc, err = call(**kwargs)
        assert rc == 1 and message in err, (kwargs, err)
    # a window whose rectangle is larger needs a larger workspace than this one's
    assert item.window_plan((0, 0, 33, 50)).ws_bytes > plan.ws_bytes
    rc, err = call(window=(0, 0, 33, 50), pitch=150)
    assert rc == 1 and "workspace below hh_jpeg_decode_window_workspace_bytes" in err


def test_a_cut_inside_the_walked_part_is_a_status_and_one_after_it_is_not(J, pkg):
    data, pixels = corpus()["420_33x50_noise_q75_plain"]
    index = J.build_jpeg_index(data)  # three MCU rows, one segment each
    info = J.jpeg_info(data)
    cut = data[:info.scan_end - 10]
    # rows 0..7 need chroma rows 0..4: MCU row 0 only; the cut lies in the last segment, after the walked part
    counts = {}
    got = J.decode_jpeg_host(cut, index=index, window=(0, 0, 8, 50), counts=counts)
    assert np.array_equal(got, pixels[:8]) and counts["segments_walked"] == 1
    # a cut inside segment 1's bytes: still after what a window of MCU row 0 walks
    inside_1 = data[:(int(index[1]["byte_offset"]) + int(index[2]["byte_offset"])) // 2]
    assert np.array_equal(J.decode_jpeg_host(inside_1, index=index, window=(2, 3, 5, 40)), pixels[2:7, 3:43])
    # the same cuts inside the walked part
    for stream, win in ((cut, (25, 0, 8, 50)), (cut, (0, 0, 33, 50)), (inside_1, (10, 0, 8, 20))):
        with pytest.raises(pkg._lib.HHError, match=r"status 3 \(bytes exhausted\)"):
            J.decode_jpeg_host(stream, index=index, window=win)


def test_cls_input_draws_the_same_geometry_for_a_jpeg_image_as_for_its_array(J, pkg, monkeypatch):
    inp = importlib.import_module(PKG + ".classification.input")
    use = ["420_120x200_scene_q90_plain", "422_21x43_scene_q90_plain", "420_130x24_noise_q90_rows1"]
    arrays = [(corpus()[n][1], i) for i, n in enumerate(use)]
    jpegs = [(J.JpegImage(corpus()[n][0]), i) for i, n in enumerate(use)]
    ci = inp.ClsInput(32)
    monkeypatch.setattr(ci, "build", lambda samples, params: params)  # the draws only: build needs the GPU
    torch.manual_seed(5)
    want = ci.train(arrays)
    torch.manual_seed(5)
    assert ci.train(jpegs) == want and all(isinstance(p, inp.CropParams) for p in want)
    assert ci.inference(jpegs) == ci.inference(arrays) == [inp.inference_geometry(*a.shape[:2], resize=ci.resize, crop=32) for a, _ in arrays]
