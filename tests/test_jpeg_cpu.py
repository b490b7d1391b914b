"""The baseline JPEG rule without a GPU: hh_debug_jpeg_encode_host (csrc/jpeg_math.h compiled for the host) against the numpy
restatement tests/jpeg_ref.py byte for byte over a grid, every stream decoded by Pillow (libjpeg) and its PSNR held against Pillow's own
encoder at the same quality and subsampling; the coverage the grid must reach; the tables against their formula and against Pillow's
DQT / DHT segments; the FDCT's bounds on the worst-case sign patterns; the size bound; the MJPEG AVI writer's layout."""
import functools
import importlib
import io
import struct

import numpy as np
import pytest

import jpeg_ref
from conftest import PKG

SIZES = [(8, 8), (17, 23), (33, 50), (64, 96), (120, 200)]
QUALITIES = [1, 30, 75, 90, 100]
SUBS = [420, 444]
CONTENTS = ["scene", "noise"]
PIL_SUB = {420: 2, 444: 0}
MARGIN_DB = 1.0  # fixed before the encoder existed, over a numpy prototype's worst case of -0.62 dB; measured: -0.67 dB (8x8 noise, quality 1, 4:2:0), profiles/jpeg.md


@pytest.fixture(scope="module")
def J(pkg):
    return importlib.import_module(PKG + ".keypoints.jpeg")


def picture(content: str, h: int, w: int) -> np.ndarray:
    rng = np.random.RandomState(h * 1000 + w)
    if content == "noise":
        return rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
    if content == "flat":
        return np.full((h, w, 3), 128, np.uint8)
    yy, xx = np.mgrid[:h, :w]
    img = np.stack([xx * 255 // max(w - 1, 1), yy * 255 // max(h - 1, 1), (xx + yy) * 255 // max(h + w - 2, 1)], -1).astype(np.uint8)
    for _ in range(6):  # random discs
        cy, cx, r = rng.randint(0, h), rng.randint(0, w), rng.randint(2, max(3, min(h, w) // 3))
        img[(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = rng.randint(0, 256, 3)
    return img


@functools.lru_cache(maxsize=None)
def reference(content: str, h: int, w: int, quality: int, sub: int):
    """computed once per case and shared"""
    return jpeg_ref.encode(picture(content, h, w), quality, sub)


def psnr(a: np.ndarray, b: np.ndarray) -> float:
    mse = np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)
    return 99.0 if mse == 0 else float(10 * np.log10(255.0 ** 2 / mse))


GRID = [(c, h, w, q, s) for (h, w) in SIZES for c in CONTENTS for q in QUALITIES for s in SUBS]


@pytest.mark.parametrize("content,h,w,quality,sub", GRID)
def test_host_equals_restatement_in_every_layout(J, content, h, w, quality, sub):
    img = picture(content, h, w)
    ref, _ = reference(content, h, w, quality, sub)
    assert J.encode_jpeg_host(img, quality, sub) == ref
    assert J.encode_jpeg_host(np.ascontiguousarray(img[..., ::-1]), quality, sub, bgr=True) == ref  # B,G,R in, true colours out
    wide = np.full((h, w + 5, 3), 77, np.uint8)
    wide[:, :w] = img
    view = wide[:, :w]
    assert view.strides[0] == 3 * (w + 5) > 3 * w
    assert J.encode_jpeg_host(view, quality, sub) == ref  # pitch > 3 w
    assert len(ref) <= J.jpeg_bound(h, w, sub)


@pytest.mark.parametrize("content,h,w,quality,sub", GRID)
def test_pillow_decodes_and_psnr_is_held(J, content, h, w, quality, sub):
    Image = pytest.importorskip("PIL.Image")
    img = picture(content, h, w)
    ours = J.encode_jpeg_host(img, quality, sub)
    dec = Image.open(io.BytesIO(ours))
    assert dec.size == (w, h) and dec.mode == "RGB"
    dec = np.asarray(dec.convert("RGB"))
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, "JPEG", quality=quality, subsampling=PIL_SUB[sub], optimize=False)
    theirs = np.asarray(Image.open(buf).convert("RGB"))
    a, b = psnr(dec, img), psnr(theirs, img)
    print(f"{content} {h}x{w} q{quality} {sub}: {a:.2f} dB, Pillow {b:.2f} dB, {a - b:+.2f}")
    assert a >= b - MARGIN_DB


def test_bgr_stream_holds_true_colours(J):
    Image = pytest.importorskip("PIL.Image")
    img = np.zeros((16, 16, 3), np.uint8)
    img[..., 0] = 255  # B,G,R: pure blue
    dec = np.asarray(Image.open(io.BytesIO(J.encode_jpeg_host(img, 95, 444, bgr=True))).convert("RGB"))
    assert dec[..., 2].min() > 240 and dec[..., 0].max() < 15


def test_grid_reaches_every_path(J):
    stats = [reference(*case)[1] for case in GRID]
    assert any(s["stuffed"] > 0 for s in stats)
    assert any(s["zrl"] > 0 for s in stats)
    assert any(s["no_eob"] > 0 for s in stats)
    wraps = [s for s in stats if s["mcu_rows"] >= 9]
    assert wraps and all(s["restarts"] == [m & 7 for m in range(s["mcu_rows"] - 1)] for s in stats)
    assert any(0 in s["restarts"][8:] for s in wraps)  # RST0 again after RST7
    flat = picture("flat", 33, 50)
    for sub in SUBS:
        ref, s = jpeg_ref.encode(flat, 90, sub)
        assert s["nonzero_ac"] == 0 and s["nonzero_dc_diff"] == 0 and s["blocks"] > 0
        assert J.encode_jpeg_host(flat, 90, sub) == ref


def test_fdct_table_equals_its_formula(J):
    got = np.zeros((8, 8), np.int64)
    for x in range(8):
        s = np.zeros((8, 8), np.int32)
        s[0, x] = 2048  # A[0][u] = (2048 T[u][x] + 1024) >> 11 = T[u][x]
        got[:, x] = J.fdct_host(s)[0][0]
    assert np.array_equal(got, jpeg_ref.T)
    assert np.all(got[0] == 5793)
    assert sorted(set(np.abs(got[1::2]).ravel())) == [1598, 4551, 6811, 8035]
    assert sorted(set(np.abs(got[[2, 6]]).ravel())) == [3135, 7568] and set(np.abs(got[4]).ravel()) == {5793}


def test_fdct_bounds_and_clamps_on_sign_patterns(J):
    """For every coefficient (v, u) the input that maximises it: s = 127 or -128 by the sign of T[v][y] T[u][x], and its negative image."""
    T = jpeg_ref.T
    rowsum = np.abs(T).sum(1).max()
    assert rowsum == 8 * 5793
    a_bound = (rowsum * 128 + 1024) >> 11
    assert a_bound == 2897
    worst_a = worst_f = worst_ac = 0
    dcs = []
    Q1 = jpeg_ref.quant_tables(100)[0]
    assert np.all(Q1 == 1)
    for v in range(8):
        for u in range(8):
            sign = np.outer(T[v], T[u]) >= 0
            for s in (np.where(sign, 127, -128), np.where(sign, -128, 127)):
                A, F = J.fdct_host(s)
                Ar, Fr = jpeg_ref.fdct(s.astype(np.int64))
                assert np.array_equal(A, Ar) and np.array_equal(F, Fr)
                worst_a, worst_f = max(worst_a, np.abs(A).max()), max(worst_f, np.abs(Fr).max())
                F64 = Fr.reshape(64)[jpeg_ref.ZZ]
                unclamped = np.sign(F64) * ((np.abs(F64) + (1 << 16)) // (1 << 17))
                worst_ac = max(worst_ac, np.abs(unclamped[1:]).max())
                dcs.append(int(unclamped[0]))
                q = jpeg_ref.quantise(Fr, Q1)
                assert np.abs(q[1:]).max() <= 1023 and -1024 <= q[0] <= 1023
    print(f"max |A| {worst_a}, max |F| 2^{np.log2(worst_f):.3f}, max |AC| {worst_ac}, DC {min(dcs)}..{max(dcs)}")
    assert worst_a <= 2896 <= a_bound and worst_f <= a_bound * rowsum < 2 ** 27.1
    assert worst_ac == 1020 and min(dcs) == -1024 and max(dcs) <= 1023  # the clamp is a guard: these images never reach it


def test_black_and_white_frames_round_trip(J):
    """DC at its extremes (-1024 at quality 100) through the whole encoder."""
    for value in (0, 255):
        img = np.full((16, 24, 3), value, np.uint8)
        for sub in SUBS:
            assert J.encode_jpeg_host(img, 100, sub) == jpeg_ref.encode(img, 100, sub)[0]


def _segments(data: bytes) -> list:
    out, i = [], 2
    while data[i + 1] != 0xDA:
        n = int.from_bytes(data[i + 2:i + 4], "big")
        out.append((data[i + 1], data[i + 4:i + 2 + n]))
        i += 2 + n
    return out


@pytest.mark.parametrize("quality", QUALITIES)
def test_tables_equal_pillows_segments(J, quality):
    Image = pytest.importorskip("PIL.Image")
    img = picture("scene", 16, 16)
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, "JPEG", quality=quality, subsampling=2, optimize=False)
    theirs, ours = _segments(buf.getvalue()), _segments(J.encode_jpeg_host(img, quality, 420))

    def tables(segs, marker, size):
        found = {}
        for m, body in segs:
            p = 0
            while m == marker and p < len(body):
                n = size(body, p)
                found[body[p]] = body[p + 1:p + n]
                p += n
        return found
    dqt = lambda b, p: 65                        # noqa: E731
    dht = lambda b, p: 17 + sum(b[p + 1:p + 17])  # noqa: E731
    assert tables(ours, 0xDB, dqt) == tables(theirs, 0xDB, dqt) and set(tables(ours, 0xDB, dqt)) == {0, 1}
    assert tables(ours, 0xC4, dht) == tables(theirs, 0xC4, dht) and set(tables(ours, 0xC4, dht)) == {0x00, 0x01, 0x10, 0x11}
    q = J.quant_tables(quality)
    assert np.array_equal(q, jpeg_ref.quant_tables(quality))
    assert bytes(int(v) for v in q[0]) == tables(theirs, 0xDB, dqt)[0] and bytes(int(v) for v in q[1]) == tables(theirs, 0xDB, dqt)[1]
    assert [m for m, _ in ours] == [0xE0, 0xDB, 0xDB, 0xC0, 0xC4, 0xC4, 0xC4, 0xC4, 0xDD]


def test_base_tables_start_as_annex_k_does(J):
    q = J.quant_tables(50)  # scale 100: the base tables
    assert list(q[0][:8]) == [16, 11, 12, 14, 12, 10, 16, 14] and list(q[1][:8]) == [17, 18, 18, 24, 21, 24, 47, 26]


def test_bound_formula_and_config(J):
    lanes, block_bits, header_bytes, _ = J.jpeg_config()
    assert (lanes, block_bits, header_bytes) == (64, 22 + 63 * 26, 629)
    for (h, w) in SIZES + [(640, 960), (16, 1120), (65535, 8)]:
        for sub in SUBS:
            m, bpm = (16, 6) if sub == 420 else (8, 3)
            rows, nblk = -(-h // m), -(-w // m) * bpm
            assert J.jpeg_bound(h, w, sub) == 629 + rows * (2 * -(-nblk * block_bits // 8) + 2)
            assert J.workspace_bytes(h, w, sub) % 16 == 0 and J.workspace_bytes(h, w, sub) >= rows * nblk * 128 + rows * 2 * -(-nblk * block_bits // 8)
    assert max(reference(*case)[1]["max_block_bits"] for case in GRID) <= block_bits


def test_refusals_by_name(J, pkg):
    img = picture("scene", 16, 16)
    HHError = pkg._lib.HHError
    for q in (0, 101):
        with pytest.raises(HHError, match="quality outside 1..100"):
            J.encode_jpeg_host(img, q, 420)
    with pytest.raises(HHError, match="subsampling must be 420 or 444"):
        J.encode_jpeg_host(img, 90, 422)
    with pytest.raises(HHError, match="output capacity below hh_jpeg_bound"):
        J.encode_jpeg_host(img, 90, 420, capacity=J.jpeg_bound(16, 16, 420) - 1)
    desc = np.zeros(1, J.DESC)
    desc[0] = (0, 0, 1 << 20, 0, 3 * 16 - 1, 16, 16, 90, 420, 0, 0)
    out, n = np.zeros(1 << 20, np.uint8), np.zeros(1, np.int64)
    assert pkg._lib.load().hh_debug_jpeg_encode_host(img.ctypes.data, desc.ctypes.data, out.ctypes.data, n.ctypes.data) == 1
    assert "pitch below 3 * w" in pkg._lib.load().hh_last_error().decode()


# ---------------------------------------------------------------- MJPEG AVI
def _walk(data: bytes, start: int, end: int) -> list:
    """[(fourcc, payload offset, size, list type or None)] of the chunks in data[start:end]; every chunk starts on an even offset"""
    out, p = [], start
    while p < end:
        assert p % 2 == 0
        cc, size = data[p:p + 4], struct.unpack("<I", data[p + 4:p + 8])[0]
        out.append((cc, p + 8, size, data[p + 8:p + 12] if cc in (b"RIFF", b"LIST") else None))
        p += 8 + size + (size & 1)
    assert p == end
    return out


def test_mjpeg_writer_layout(J, tmp_path):
    Image = pytest.importorskip("PIL.Image")
    h, w, fps = 24, 40, 25
    frames, n = [], 0
    while not (len(frames) >= 3 and {len(f) & 1 for f in frames[:3]} == {0, 1}):  # odd and even lengths among the first three
        frames.insert(0, J.encode_jpeg_host(picture("scene", h, w) + np.uint8(n), 60 + n, 420))
        n += 1
        assert n < 40
    frames = frames[:3]
    path = tmp_path / "clip.avi"
    with J.MJPEGWriter(path, fps, w, h) as wr:
        for f in frames:
            wr.write(f)
    with pytest.raises(ValueError):
        wr.write(frames[0])  # closed
    data = path.read_bytes()
    (riff,) = _walk(data, 0, len(data))
    assert riff[0] == b"RIFF" and riff[3] == b"AVI " and riff[2] == len(data) - 8
    top = _walk(data, 12, len(data))
    assert [(c[0], c[3]) for c in top] == [(b"LIST", b"hdrl"), (b"LIST", b"movi"), (b"idx1", None)]
    hdrl, movi, idx1 = top
    inner = _walk(data, hdrl[1] + 4, hdrl[1] + hdrl[2])
    assert [(c[0], c[2], c[3]) for c in inner] == [(b"avih", 56, None), (b"LIST", inner[1][2], b"strl")]
    avih = struct.unpack("<14I", data[inner[0][1]:inner[0][1] + 56])
    assert avih[0] == 1000000 // fps and avih[3] & 0x10 and avih[4] == 3 and avih[6] == 1 and avih[8:10] == (w, h)
    strl = _walk(data, inner[1][1] + 4, inner[1][1] + inner[1][2])
    assert [(c[0], c[2]) for c in strl] == [(b"strh", 56), (b"strf", 40)]
    strh = data[strl[0][1]:strl[0][1] + 56]
    assert strh[:8] == b"vidsMJPG" and struct.unpack("<II", strh[20:28]) == (1, fps) and struct.unpack("<I", strh[32:36])[0] == 3
    strf = struct.unpack("<IiiHH4sIiiII", data[strl[1][1]:strl[1][1] + 40])
    assert strf[:6] == (40, w, h, 1, 24, b"MJPG")
    chunks = _walk(data, movi[1] + 4, movi[1] + movi[2])
    assert [c[0] for c in chunks] == [b"00dc"] * 3 and [c[2] for c in chunks] == [len(f) for f in frames]
    for (cc, at, size, _), f in zip(chunks, frames):
        assert data[at:at + size] == f
        if size & 1:
            assert data[at + size] == 0
        dec = Image.open(io.BytesIO(data[at:at + size]))
        dec.load()
        assert dec.size == (w, h)
    assert idx1[2] == 16 * 3
    for k, (cc, at, size, _) in enumerate(chunks):
        e = struct.unpack("<4sIII", data[idx1[1] + 16 * k:idx1[1] + 16 * k + 16])
        assert e == (b"00dc", 0x10, at - 8 - movi[1], size)  # offset of the chunk header from the 'movi' fourcc
        assert data[movi[1] + e[2]:movi[1] + e[2] + 4] == b"00dc"


def test_mjpeg_writer_refuses_to_pass_4gb(J, tmp_path):
    wr = J.MJPEGWriter(tmp_path / "big.avi", 30, 8, 8)
    wr._pos = (1 << 32) - 700  # as if that much had been written
    with pytest.raises(ValueError, match="4 GB"):
        wr.write(J.encode_jpeg_host(picture("scene", 8, 8), 90, 420))
    wr._pos = wr._movi + 4
    wr.close()
    with pytest.raises(ValueError, match="not a JPEG"):
        J.MJPEGWriter(tmp_path / "x.avi", 30, 8, 8).write(b"nope")
