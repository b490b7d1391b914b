"""The JPEG index built by self-synchronising lanes, on the host (no GPU): hh_debug_jpeg_index_sync_host, which runs the shared code
of the device index (csrc/jpeg_dec_math.h: jpeg_idx_walk) with `lanes` subsequences per round, against hh_jpeg_index_host
(build_jpeg_index), entry for entry and byte for byte; its statuses on malformed streams; every refusal by name; what
JpegImage(index="device") is and stages."""
import ctypes as C
import functools
import importlib
import io

import numpy as np
import pytest

from conftest import PKG
from test_jpeg_decode_cpu import corpus, names

SUBSEQ = (4, 16, 64, 128)
LANES = (64, 1024)


@pytest.fixture(scope="module")
def J(pkg):
    return importlib.import_module(PKG + ".keypoints.jpeg")


def restartless(J) -> list[str]:
    return [n for n in names() if not J.jpeg_info(corpus()[n][0]).restart_interval]


def host_status(J, pkg, data) -> int:
    """The code hh_jpeg_index_host meets on this stream (0: it walks), read from its refusal."""
    try:
        J.build_jpeg_index(data, 1)
        return 0
    except pkg._lib.HHError as e:
        assert "the scan cannot be walked: " in str(e), str(e)
        return J.STATUS_NAMES.index(str(e).split("the scan cannot be walked: ")[1])


def assert_parity(J, data, label):
    info = J.jpeg_info(data)
    for mps in (1, 2, 3, 8, info.mcu_cols):
        want = J.build_jpeg_index(data, mps)
        for sub in SUBSEQ:
            for lanes in LANES:
                got, status, counts = J.index_sync_host(data, mps, sub, lanes)
                where = (label, mps, sub, lanes)
                assert status == 0 and got.dtype == want.dtype and len(got) == len(want), where
                assert got.tobytes() == want.tobytes(), (where, [i for i in range(len(want)) if got[i] != want[i]][:3])
                assert counts["subsequences"] == max(1, -(-(info.scan_end - info.scan_offset) // sub)), where
                # (a round less where the image's last block ends before the last round's subsequences, which then hold padding only)
                assert -(-counts["subsequences"] // lanes) - 1 <= counts["rounds"] <= -(-counts["subsequences"] // lanes) and counts["rounds"] >= 1, where
                assert counts["iterations"] <= counts["subsequences"] and counts["iterations_worst"] <= min(lanes, counts["subsequences"]), where
                assert counts["blocks_true"] == info.mcu_cols * info.mcu_rows * (1 if info.components == 1 else {444: 3, 422: 4, 420: 6}[info.sampling]), where
                assert counts["blocks_decoded"] >= counts["blocks_true"], where


def test_corpus_parity(J):
    found = restartless(J)
    assert len(found) >= 40
    assert {J.jpeg_info(corpus()[n][0]).sampling for n in found} == {420, 422, 444, 400}
    assert any("optimize" in n for n in found) and any("q16" in n for n in found)
    # (the corpus's largest scan has fewer than 1024 four-byte subsequences: round boundaries are reached through lanes=64)
    assert max(-(-(J.jpeg_info(corpus()[n][0]).scan_end - J.jpeg_info(corpus()[n][0]).scan_offset) // 4) for n in found) > 64
    for n in found:
        assert_parity(J, corpus()[n][0], n)


@functools.lru_cache(maxsize=None)
def stress_streams() -> dict:
    """Pillow-written streams: noise at quality 100 (long codes) and quality 1 (blocks of a few bits, dozens per subsequence), a smooth
    ramp; 4:2:0 / 4:4:4 / grayscale; optimised tables.  Made once, shared read-only."""
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(11)
    out = {}
    for h, w in ((64, 64), (120, 200)):
        noise = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        ramp = np.stack([np.add.outer(np.arange(h) * 2, np.arange(w)) % 256] * 3, axis=2).astype(np.uint8)
        ramp[..., 1] = ramp[..., 1][::-1]
        for content, pixels in (("noise", noise), ("ramp", ramp)):
            for quality in (100, 1) if content == "noise" else (90,):
                for sampling, mode, sub in ((420, "RGB", 2), (444, "RGB", 0), (400, "L", None)):
                    for optimize in (False, True):
                        if optimize and (sampling != 420 or (h, w) != (64, 64)):
                            continue
                        f = io.BytesIO()
                        img = Image.fromarray(pixels if mode == "RGB" else pixels[..., 0].copy(), mode)
                        kw = {} if sub is None else {"subsampling": sub}
                        img.save(f, "JPEG", quality=quality, optimize=optimize, **kw)
                        out[f"{sampling}_{h}x{w}_{content}_q{quality}{'_optimize' if optimize else ''}"] = f.getvalue()
    return out


def test_pillow_written_stress_streams(J):
    streams = stress_streams()
    assert len(streams) >= 20
    for label, data in streams.items():
        assert_parity(J, data, label)
    # quality 1 noise: dozens of blocks per 128-byte subsequence; quality 100 noise: less than one per 64-byte subsequence (the mean
    # block is longer than a subsequence: lanes that decode no block at all, and exits past the next lane's subsequence)
    info = J.jpeg_info(streams["444_120x200_noise_q1"])
    assert 3 * info.mcu_cols * info.mcu_rows / -(-(info.scan_end - info.scan_offset) // 128) > 24
    info = J.jpeg_info(streams["444_120x200_noise_q100"])
    assert 3 * info.mcu_cols * info.mcu_rows / -(-(info.scan_end - info.scan_offset) // 64) < 1


def substitutions(data: bytes, info):
    """The fixed single-byte substitutions of test_jpeg_decode_cpu.bad_code_stream (what tests/test_gpu_jpeg_decode.py uses), all of them."""
    for at in range(info.scan_offset + 8, info.scan_end - 8, 7):
        for value in (0xfe, 0xfd, 0x7f):
            if data[at] == 0xff or data[at - 1] == 0xff:
                continue
            yield data[:at] + bytes([value]) + data[at + 1:]


def test_malformed_streams_end_in_the_hosts_status(J, pkg):
    small = ["420_17x23_scene_q90_plain", "444_17x23_noise_q30_plain", "400_17x23_noise_q75_plain"]
    seen = set()
    ncases = 0
    for name in small:
        data = corpus()[name][0]
        info = J.jpeg_info(data)
        trials = [data[:n] for n in range(len(data))] + list(substitutions(data, info))
        if name == small[0]:
            noise = corpus()["420_33x50_noise_q75_plain"][0]
            trials += list(substitutions(noise, J.jpeg_info(noise)))
        for k, trial in enumerate(trials):
            try:
                cut = J.jpeg_info(trial)
            except pkg._lib.HHError:
                for sub, lanes in ((4, 64), (128, 1024)):  # refused by name by both, before any walk
                    with pytest.raises(pkg._lib.HHError):
                        J.index_sync_host(trial, 1, sub, lanes)
                continue
            want = host_status(J, pkg, trial)
            seen.add(want)
            for sub, lanes in ((4, 64), (4, 7), (16, 64), (128, 1024)):
                got, status, counts = J.index_sync_host(trial, 1, sub, lanes)
                assert status == want, (name, k, sub, lanes, status, want)
                assert (len(got) == 0) == (status != 0)
                assert counts["iterations"] <= counts["subsequences"] == max(1, -(-(min(cut.scan_end, len(trial)) - cut.scan_offset) // sub))
                if not status:
                    assert got.tobytes() == J.build_jpeg_index(trial, 1).tobytes()
                ncases += 1
    assert seen >= {0, 1, 3} and ncases > 2000, (seen, ncases)


def test_refusals_by_name(J, pkg, monkeypatch):
    HHError = pkg._lib.HHError
    data = corpus()["420_33x50_scene_q90_plain"][0]
    lanes, default, minimum, mps = J.index_config()
    assert (lanes, default, minimum, mps) == (1024, 32, 4, 2) and default % 4 == 0
    with pytest.raises(HHError, match="subseq_bytes below the minimum"):
        J.index_sync_host(data, 1, minimum - 4, 64)
    with pytest.raises(HHError, match="subseq_bytes must be a multiple of 4"):
        J.index_sync_host(data, 1, 6, 64)
    with pytest.raises(HHError, match="mcus_per_segment must be at least 1"):
        J.index_sync_host(data, 0, 16, 64)
    with pytest.raises(HHError, match="capacity below the number of segments"):
        J.index_sync_host(data, 1, 16, 64, capacity=len(J.build_jpeg_index(data, 1)) - 1)
    with pytest.raises(HHError, match="lanes must lie in"):
        J.index_sync_host(data, 1, 16, 0)
    rows = corpus()["420_33x50_scene_q90_rows1"][0]
    with pytest.raises(HHError, match="restart interval"):
        J.index_sync_host(rows, 1, 16, 64)
    lib = pkg._lib.load()
    info = J._parse(J._bytes_view(data))
    assert lib.hh_jpeg_index_workspace_bytes(info.ctypes.data, 128) == 0
    assert lib.hh_jpeg_index_workspace_bytes(info.ctypes.data, 2) == -1 and "below the minimum" in lib.hh_last_error().decode()
    # a device-indexed image has no offsets on the host
    item = J.JpegImage(data, index="device")
    with pytest.raises(ValueError, match="window decode needs the segments' offsets on the host"):
        item.window_plan((0, 0, 8, 8))
    with pytest.raises(ValueError, match="`windows` with a device-indexed stream"):
        J.decode_jpeg_device([data], "device", windows=[(0, 0, 8, 8)])
    with pytest.raises(ValueError, match="mcus_per_segment must be at least 1"):
        J.JpegImage(data, index="device", mcus_per_segment=0)
    with pytest.raises(ValueError, match="is not 'device'"):
        J.JpegImage(data, index="host")
    with pytest.raises(ValueError, match="share one mcus_per_segment"):
        J.decode_jpeg_device([item, J.JpegImage(data, index="device", mcus_per_segment=8)])
    ti_mod = importlib.import_module(PKG + ".keypoints.train_input")
    ti = ti_mod.TrainInput(64, [1 / 4, 1 / 2], device="cpu")
    with pytest.raises(ValueError, match="TrainInput.build: a device-indexed JpegImage"):
        ti.build([(item, np.zeros(item.shape[:2], bool), np.zeros((0, 17, 3), np.float32))], [None])
    ci_mod = importlib.import_module(PKG + ".classification.input")
    with pytest.raises(ValueError, match="ClsInput.build: a device-indexed JpegImage"):
        ci_mod.ClsInput(16, device="cpu").build([(item, 0)], [(16, 24, 0, 5)])


def test_dri_streams_and_the_blank_table_block(J, pkg):
    lib = pkg._lib.load()
    # a DRI stream given index="device" keeps its restart segments
    rows = corpus()["420_33x50_scene_q90_rows1"][0]
    item = J.JpegImage(rows, index="device")
    assert not item.device_index and item.segments is not None and item.segments.tobytes() == J.JpegImage(rows).segments.tobytes()
    assert int(item.info[0]["reserved"][1]) == 0
    for name in ("420_33x50_noise_q75_plain", "400_17x23_scene_q90_plain", "422_21x43_noise_q90_plain"):
        data = corpus()[name][0]
        for mps in (1, 2, 5):
            item = J.JpegImage(data, index="device", mcus_per_segment=mps)
            host = J.JpegImage(data, J.build_jpeg_index(data, mps))
            assert item.device_index and item.segments is None and item.nseg == host.nseg and item.tables_bytes == host.tables_bytes
            assert item.shape == host.shape and item.staged_bytes() == host.staged_bytes()
            a, b = np.full(item.staged_bytes(), 0xa5, np.uint8), np.full(item.staged_bytes(), 0xa5, np.uint8)
            assert item.stage(a, 0) == host.stage(b, 0)
            tables_at = item.stage(a, 0)[1]
            ia, ib = a[tables_at:tables_at + J.INFO.itemsize].view(J.INFO)[0], b[tables_at:tables_at + J.INFO.itemsize].view(J.INFO)[0]
            assert list(ia["reserved"]) == [0, 1, 0] and list(ib["reserved"]) == [0, 0, 0]
            ia["reserved"][1] = 0
            seg_at = tables_at + item.tables_bytes - J.SEGMENT.itemsize * item.nseg
            assert a[:seg_at].tobytes() == b[:seg_at].tobytes()  # the stream, the info, the quantiser and Huffman tables
            ea, eb = a[seg_at:seg_at + 32 * item.nseg].view(J.SEGMENT), b[seg_at:seg_at + 32 * item.nseg].view(J.SEGMENT)
            assert np.array_equal(ea["first_mcu"], eb["first_mcu"]) and np.array_equal(ea["mcu_count"], eb["mcu_count"])
            for field in ("byte_offset", "bit_offset", "pred", "byte_end"):
                assert not ea[field].any()
    n = C.c_int(0)
    out = np.zeros(1 << 16, np.uint8)
    assert lib.hh_jpeg_index_tables(J._bytes_view(rows).ctypes.data, len(rows), 2, out.ctypes.data, out.size, C.byref(n)) == 1
    assert "restart interval" in lib.hh_last_error().decode()
    assert lib.hh_jpeg_index_tables(J._bytes_view(data).ctypes.data, len(data), 0, out.ctypes.data, out.size, C.byref(n)) == 1
    assert "mcus_per_segment must be at least 1" in lib.hh_last_error().decode()
    assert lib.hh_jpeg_index_tables(J._bytes_view(data).ctypes.data, len(data), 1, out.ctypes.data, 7920, C.byref(n)) == 1
    assert "room below hh_jpeg_decode_tables_bytes" in lib.hh_last_error().decode()
