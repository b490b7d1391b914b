"""The JPEG decoder's rule on the host (no GPU): hh_debug_jpeg_decode_host == the numpy restatement (tests/jpeg_decode_ref.py) == Pillow's
pixels of tests/golden/jpeg_decode.npz, byte for byte, on every corpus entry; decoding from an index at several segment sizes; every
refusal by name; MJPEGWriter -> MJPEGReader."""
import functools
import importlib
import json
import os
import struct

import numpy as np
import pytest

import jpeg_decode_ref as ref
from conftest import PKG

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def J(pkg):
    return importlib.import_module(PKG + ".keypoints.jpeg")


@functools.lru_cache(maxsize=None)
def corpus():
    """{name: (stream bytes, Pillow's pixels)}, loaded once and shared (read only)."""
    z = np.load(os.path.join(GOLDEN, "jpeg_decode.npz"))
    with open(os.path.join(GOLDEN, "jpeg_decode_meta.json")) as f:
        meta = json.load(f)
    out = {e["name"]: (z["s_" + e["name"]].tobytes(), z["p_" + e["name"]]) for e in meta["entries"]}
    for _, p in out.values():
        p.setflags(write=False)
    return out


def names():
    with open(os.path.join(GOLDEN, "jpeg_decode_meta.json")) as f:
        return [e["name"] for e in json.load(f)["entries"]]


@functools.lru_cache(maxsize=None)
def restated(name: str):
    return ref.decode(corpus()[name][0], with_preds=True)


def test_corpus_holds_what_the_issue_lists():
    with open(os.path.join(GOLDEN, "jpeg_decode_meta.json")) as f:
        entries = json.load(f)["entries"]
    have = {(e["sampling"], e["h"], e["w"]) for e in entries}
    for want in [(420, 1, 1), (420, 8, 8), (420, 16, 4), (420, 16, 5), (420, 17, 23), (420, 33, 50), (420, 36, 44), (420, 130, 24), (422, 9, 37),
                 (422, 21, 43), (422, 8, 4), (444, 17, 23), (400, 17, 23)]:
        assert want in have, want
    assert {e["quality"] for e in entries} >= {1, 30, 75, 90, 100}
    assert {e["variant"] for e in entries} >= {"plain", "optimize", "q16", "rows1", "blocks3", "own"}
    assert {e["content"] for e in entries} == {"scene", "noise", "flat"}
    assert any(e["variant"] == "own" and e["h"] == 130 for e in entries)  # RSTm wraps past 7
    assert os.path.getsize(os.path.join(GOLDEN, "jpeg_decode.npz")) < 1 << 20


@pytest.mark.parametrize("name", names())
def test_host_equals_restatement_equals_pillow(J, name):
    data, pixels = corpus()[name]
    got = J.decode_jpeg_host(data)
    assert got.shape == pixels.shape and np.array_equal(got, pixels), np.argwhere(got != pixels)[:4]
    assert np.array_equal(restated(name)[0], pixels)


def test_bgr_swaps_the_stores(J):
    data, pixels = corpus()["420_33x50_scene_q90_plain"]
    assert np.array_equal(J.decode_jpeg_host(data, bgr=True), pixels[:, :, ::-1])
    assert np.array_equal(ref.decode(data, bgr=True), pixels[:, :, ::-1])


def test_golden_file_is_what_pillow_gives_today(J):
    """When Pillow imports, the corpus is regenerated in memory and must equal the file."""
    pytest.importorskip("PIL")
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(GOLDEN), "..", "tools"))
    try:
        tool = importlib.import_module("make_jpeg_decode_golden")
    finally:
        sys.path.pop(0)
    arrays, meta = tool.make(J)
    have = corpus()
    assert [e["name"] for e in meta] == names()
    for e in meta:
        assert arrays["s_" + e["name"]].tobytes() == have[e["name"]][0], e["name"]
        assert np.array_equal(arrays["p_" + e["name"]], have[e["name"]][1]), e["name"]


@pytest.mark.parametrize("name", ["420_33x50_noise_q75_plain", "420_130x24_scene_q90_plain", "422_21x43_noise_q90_plain", "444_17x23_noise_q30_plain",
                                  "400_17x23_noise_q75_plain", "420_33x50_noise_q75_optimize", "420_33x50_noise_q90_blocks3", "420_130x24_noise_q90_rows1"])
def test_decoding_from_an_index(J, name):
    """Segments of 1 MCU, 3 MCUs, one MCU row and the whole image give the same bytes; every entry's DC predictors are the restatement's
    running predictors at its first MCU, and the entries tile the MCU grid."""
    data, pixels = corpus()[name]
    _, preds, H = restated(name)
    nmcu = H.mcols * H.mrows
    for mps in (1, 3, H.mcols, nmcu):
        index = J.build_jpeg_index(data, mps)
        assert index["first_mcu"][0] == 0 and int(index["mcu_count"].sum()) == nmcu
        assert np.array_equal(index["first_mcu"][1:], np.cumsum(index["mcu_count"])[:-1])
        assert int(index["mcu_count"].max()) <= mps
        if not H.ri:
            assert len(index) == -(-nmcu // mps)
        assert np.array_equal(index["pred"], preds[index["first_mcu"]]), mps
        assert np.array_equal(J.decode_jpeg_host(data, index=index), pixels), mps
    assert np.array_equal(J.build_jpeg_index(data), J.build_jpeg_index(data, H.mcols))  # the default: one MCU row


def test_info(J):
    i = J.jpeg_info(corpus()["422_21x43_noise_q90_rows1"][0])
    assert (i.h, i.w, i.components, i.sampling, i.restart_interval, i.mcu_cols, i.mcu_rows) == (21, 43, 3, 422, 3, 3, 3)
    i = J.jpeg_info(corpus()["400_17x23_scene_q90_plain"][0])
    assert (i.h, i.w, i.components, i.sampling, i.restart_interval) == (17, 23, 1, 400, 0)


def _find(data: bytes, marker: int) -> int:
    """The offset of the first segment with this marker in the header."""
    at = 2
    while True:
        assert data[at] == 0xff
        if data[at + 1] == marker:
            return at
        if data[at + 1] == 0xda:
            raise IndexError(marker)
        at += 2 + (data[at + 2] << 8 | data[at + 3])


def _patch(data: bytes, at: int, value: int) -> bytes:
    return data[:at] + bytes([value]) + data[at + 1:]


def _drop(data: bytes, marker: int) -> bytes:
    while True:
        try:
            at = _find(data, marker)
        except (AssertionError, IndexError):
            return data
        data = data[:at] + data[at + 2 + (data[at + 2] << 8 | data[at + 3]):]
        if marker == 0xda:
            return data


def test_every_refusal_by_name(J, pkg):
    HHError = pkg._lib.HHError
    good = corpus()["420_33x50_scene_q90_plain"][0]
    sof, sos = _find(good, 0xc0), _find(good, 0xda)
    adobe = b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00\x00"
    eoi = good.rindex(b"\xff\xd9")
    cases = [
        (_patch(good, sof + 1, 0xc2), "progressive"),
        (_patch(good, sof + 1, 0xc1), "only baseline streams \\(SOF0\\)"),
        (_patch(good, sof + 1, 0xc9), "arithmetic coding"),
        (good[:sof] + b"\xff\xcc\x00\x04\x00\x00" + good[sof:], "arithmetic coding"),
        (_patch(good, sof + 4, 12), "12-bit precision"),
        (_patch(good, sof + 9, 4), "4 components"),
        (_patch(good, sof + 11, 0x12), "unsupported sampling"),   # 4:4:0
        (_patch(good, sof + 11, 0x41), "unsupported sampling"),   # 4:1:1
        (_patch(good, sos + 4, 1), "more than one scan"),
        (good[:eoi] + good[sos:eoi] + good[eoi:], "more than one scan"),
        (good[:sof] + adobe + good[sof:], "Adobe marker with transform 0"),
        (_drop(good, 0xc4), "missing tables"),
        (_drop(good, 0xdb), "missing tables"),
        (_patch(_patch(good, sof + 5, 0), sof + 6, 0), "dimension of 0"),
        (_patch(_patch(good, sof + 7, 0), sof + 8, 0), "dimension of 0"),
        (good[:sof + 5] + b"\xff\xff\xff\xff" + good[sof + 9:], "beyond what int32 offsets allow"),
        (good[:sos + 3], "truncated header"),
        (good[:sof + 6], "truncated header"),
        (good[:3], "truncated header"),
        (b"\x00" + good[1:], "not a JPEG stream"),
    ]
    for data, message in cases:
        for call in (J.jpeg_info, J.build_jpeg_index, J.decode_jpeg_host, J.JpegImage):
            with pytest.raises(HHError, match=message):
                call(data)
    # the Adobe marker with transform 1 (YCbCr) and APPn / COM segments are skipped
    ok = good[:sof] + adobe[:-1] + b"\x01" + b"\xff\xfe\x00\x05abc" + good[sof:]
    assert np.array_equal(J.decode_jpeg_host(ok), corpus()["420_33x50_scene_q90_plain"][1])
    # a stream the index pass cannot walk is refused by name as well
    scan = J.jpeg_info(good).scan_offset
    with pytest.raises(HHError, match="the scan cannot be walked"):
        J.build_jpeg_index(good[:scan + 40] + good[eoi:])
    # restart markers out of step with the interval
    rows = corpus()["420_33x50_scene_q90_rows1"][0]
    first = rows.index(b"\xff\xd0", J.jpeg_info(rows).scan_offset)
    with pytest.raises(HHError, match="restart marker"):
        J.jpeg_info(_patch(rows, first + 1, 0x00))
    with pytest.raises(HHError, match="out of sequence"):
        J.decode_jpeg_host(_patch(rows, first + 1, 0xd3))


def test_malformed_scans_end_in_a_status(J, pkg):
    """What the GPU test's two malformed streams are on the host: a truncated scan, and a substituted byte the decoder meets as a bad code."""
    HHError = pkg._lib.HHError
    cut, index = truncated_stream(J)
    with pytest.raises(HHError, match="status 3 \\(bytes exhausted\\)"):
        J.decode_jpeg_host(cut, index=index)
    bad, at = bad_code_stream(J, pkg)
    assert at > 0
    with pytest.raises(HHError, match="status 1 \\(bad Huffman code\\)"):
        J.decode_jpeg_host(bad)


def truncated_stream(J):
    """The noise corpus entry cut 10 bytes before its EOI, with the index of the whole stream: only the last segment runs dry."""
    data = corpus()["420_33x50_noise_q75_plain"][0]
    return data[:J.jpeg_info(data).scan_end - 10], J.build_jpeg_index(data)


def bad_code_stream(J, pkg):
    """The noise corpus entry with the first single scan byte substituted (fixed values, in order) that makes the host decoder report status 1."""
    data = corpus()["420_33x50_noise_q75_plain"][0]
    info = J.jpeg_info(data)
    index = J.build_jpeg_index(data)
    for at in range(info.scan_offset + 8, info.scan_end - 8, 7):
        for value in (0xfe, 0xfd, 0x7f):
            if data[at] == 0xff or data[at - 1] == 0xff:
                continue
            trial = data[:at] + bytes([value]) + data[at + 1:]
            try:
                J.decode_jpeg_host(trial, index=index)
            except pkg._lib.HHError as e:
                if "status 1" in str(e):
                    return trial, at
    return None, -1


def test_index_cache(J, tmp_path):
    data = corpus()["420_33x50_scene_q90_plain"][0]
    path = tmp_path / "a.jpg"
    path.write_bytes(data)
    cache = J.JpegIndexCache()
    a = cache.get(path)
    assert cache.get(path) is a and len(cache) == 1
    assert np.array_equal(a, J.build_jpeg_index(data))
    other = corpus()["420_17x23_scene_q90_plain"][0]
    path.write_bytes(other)
    os.utime(path, ns=(1, 1))
    b = cache.get(path)
    assert b is not a and np.array_equal(b, J.build_jpeg_index(other))


def test_mjpeg_reader_inverts_the_writer(J, tmp_path):
    from test_jpeg_cpu import picture
    frames = [J.encode_jpeg_host(np.roll(picture("scene", 24, 40), 3 * i, axis=1), 90, 420) for i in range(3)]
    frames.append(frames[0][:-2] + b"\x00\xff\xd9")  # an odd length next to even ones: chunk padding
    path = tmp_path / "clip.avi"
    with J.MJPEGWriter(path, 25, 40, 24) as wr:
        for f in frames:
            wr.write(f)
    rd = J.MJPEGReader(path)
    assert len(rd) == 4 and rd.fps == 25 and (rd.width, rd.height) == (40, 24)
    assert list(rd) == frames and rd[2] == frames[2]
    raw = path.read_bytes()
    for cut, message in ((16, "truncated"), (5, "truncated"), (16 * 4 + 8, "idx1")):
        (tmp_path / "cut.avi").write_bytes(raw[:-cut])
        with pytest.raises(ValueError, match=message):
            J.MJPEGReader(tmp_path / "cut.avi")
    # idx1 cut short with its size field patched to match: the frame count of the header gives it away
    at = raw.rindex(b"idx1")
    short = raw[:at + 4] + struct.pack("<I", 48) + raw[at + 8:at + 8 + 48]
    (tmp_path / "short.avi").write_bytes(short)
    with pytest.raises(ValueError, match="truncated 'idx1'"):
        J.MJPEGReader(tmp_path / "short.avi")
    (tmp_path / "other.avi").write_bytes(raw.replace(b"vidsMJPG", b"vidsH264"))
    with pytest.raises(ValueError, match="not an MJPG AVI"):
        J.MJPEGReader(tmp_path / "other.avi")
    (tmp_path / "not.avi").write_bytes(b"RIFF" + raw[4:8] + b"WAVE" + raw[12:])
    with pytest.raises(ValueError, match="not a RIFF AVI"):
        J.MJPEGReader(tmp_path / "not.avi")
