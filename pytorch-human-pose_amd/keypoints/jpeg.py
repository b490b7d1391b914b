"""The files the reference's video and directory paths end in, without cv2: baseline JPEG encoded on the GPU from the rendered frames and
figures where they already are (hh_jpeg_encode_u8_batch: one call of three launches for a batch of mixed sizes; the rule is written at
that entry point in include/hhrnet.h), and the Motion-JPEG AVI of `cv2.VideoWriter(..., "MJPG", ...)` (src/base/datasets/video.py:93-106)
as a pure-Python RIFF writer.  Only compressed bytes cross to the host.  There is no CPU fallback: `encode_jpeg_host` is the same rule
compiled for the host, for tests.
"""
from __future__ import annotations

import ctypes as C
import struct

import numpy as np
import torch

from .. import _lib

# hh_jpeg_desc of include/hhrnet.h
DESC = np.dtype([("src_offset", "<i8"), ("out_offset", "<i8"), ("out_capacity", "<i8"), ("ws_offset", "<i8"), ("pitch", "<i8"), ("h", "<i4"),
                 ("w", "<i4"), ("quality", "<i4"), ("subsampling", "<i4"), ("flags", "<i4"), ("reserved", "<i4")])
assert DESC.itemsize == 64
FLAG_BGR = 1


def _per_frame(value, n: int) -> list:
    return list(value) if isinstance(value, (list, tuple)) else [value] * n


def _subsampling(s) -> int:
    """"420" / "444" / 420 / 444 -> the integer; anything else goes to the library as it is and is refused there by name."""
    try:
        return int(s)
    except (TypeError, ValueError):
        raise ValueError(f"subsampling {s!r} is not '420' or '444'") from None


def jpeg_bound(h: int, w: int, subsampling=420) -> int:
    """hh_jpeg_bound: the worst-case bytes of the stream of one h x w frame."""
    n = _lib.load().hh_jpeg_bound(int(h), int(w), _subsampling(subsampling))
    if n < 0:
        _lib.check(1)
    return int(n)


def workspace_bytes(h: int, w: int, subsampling=420) -> int:
    n = _lib.load().hh_jpeg_workspace_bytes(int(h), int(w), _subsampling(subsampling))
    if n < 0:
        _lib.check(1)
    return int(n)


def quant_tables(quality: int) -> np.ndarray:
    """hh_jpeg_quant_tables: int32 [2,64], luminance and chrominance divisors in zigzag order."""
    out = np.zeros((2, 64), np.int32)
    _lib.check(_lib.load().hh_jpeg_quant_tables(int(quality), out.ctypes.data))
    return out


def jpeg_config() -> tuple[int, int, int, int]:
    """(blocks per pass of the entropy kernel, per-block bound in bits, header bytes, MCUs per transform workgroup)."""
    cfg = (C.c_int * 4)()
    _lib.check(_lib.load().hh_jpeg_config(cfg))
    return tuple(cfg)


def fdct_host(samples: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """hh_debug_jpeg_fdct: the row pass A and the column pass F of one [8,8] block of samples (tests)."""
    s = np.ascontiguousarray(samples, dtype=np.int32).reshape(64)
    a, f = np.zeros(64, np.int32), np.zeros(64, np.int32)
    _lib.check(_lib.load().hh_debug_jpeg_fdct(s.ctypes.data, a.ctypes.data, f.ctypes.data))
    return a.reshape(8, 8), f.reshape(8, 8)


def _pitched(a: np.ndarray) -> bool:
    return a.ndim == 3 and a.shape[2] == 3 and a.dtype == np.uint8 and a.strides[2] == 1 and a.strides[1] == 3 and a.strides[0] >= 3 * a.shape[1]


def encode_jpeg_host(image: np.ndarray, quality: int = 90, subsampling="420", bgr: bool = False, capacity: int | None = None) -> bytes:
    """hh_debug_jpeg_encode_host: one frame through the rule compiled for the host (tests and the GPU tests' yardstick; needs the library,
    no GPU).  `image`: uint8 [h,w,3], rows may be `pitch` bytes apart (a column slice of a wider array)."""
    image = np.asarray(image)
    if not _pitched(image):
        image = np.ascontiguousarray(image, dtype=np.uint8)
        if image.ndim != 3 or image.shape[2] != 3:
            raise ValueError("encode_jpeg_host: a uint8 [h,w,3] array is needed")
    h, w = image.shape[:2]
    lib = _lib.load()
    sub = _subsampling(subsampling)
    bound = lib.hh_jpeg_bound(h, w, sub)
    cap = max(int(bound), 1) if capacity is None else int(capacity)
    desc = np.zeros(1, DESC)
    desc[0] = (0, 0, cap, 0, image.strides[0], h, w, int(quality), sub, FLAG_BGR if bgr else 0, 0)
    out = np.empty(cap, np.uint8)
    length = C.c_longlong(0)
    _lib.check(lib.hh_debug_jpeg_encode_host(image.ctypes.data, desc.ctypes.data, out.ctypes.data, C.byref(length)))
    return out[:length.value].tobytes()


def _align(n: int, a: int = 64) -> int:
    return (n + a - 1) // a * a


def encode_jpeg_device(frames: list, quality=90, subsampling="420", bgr=False, capacity=None) -> list[bytes]:
    """One hh_jpeg_encode_u8_batch, on the current stream, for a batch of frames of mixed sizes -> one JFIF stream (bytes) per frame.
    `frames`: uint8 [h,w,3], each a device tensor (read in place; a view whose rows are `pitch` >= 3 w bytes apart is allowed) or a numpy
    array (uploaded here through the one pinned block that also carries the descriptors).  `quality` (1..100; 90 is a parameter, not a
    measured optimum), `subsampling` ("420" or "444") and `bgr` (the frame is B,G,R: the stream still holds the true colours): one
    value, or a list with one per frame.  Two device-to-host copies: the n lengths, then exactly the encoded bytes.
    `capacity`: the room given to every stream instead of its hh_jpeg_bound (a smaller one is refused by the library before any launch)."""
    n = len(frames)
    if n == 0:
        return []
    lib = _lib.load()
    quals, subs, bgrs = _per_frame(quality, n), [_subsampling(s) for s in _per_frame(subsampling, n)], _per_frame(bgr, n)
    on_dev = [isinstance(f, torch.Tensor) for f in frames]
    device = next((f.device for f in frames if isinstance(f, torch.Tensor)), None) or torch.device("cuda", torch.cuda.current_device())
    at = _align(DESC.itemsize * n)
    src_at, pitches = [], []
    for f, dev in zip(frames, on_dev):
        if dev:
            if not (f.dtype == torch.uint8 and f.dim() == 3 and f.shape[2] == 3 and f.device == device and f.stride(2) == 1 and f.stride(1) == 3
                    and f.stride(0) >= 3 * f.shape[1]):
                raise ValueError("a device frame must be a uint8 [h,w,3] tensor (or a view of one with whole pixels and a row pitch) on one device")
            src_at.append(None)
            pitches.append(int(f.stride(0)))
        else:
            if not (isinstance(f, np.ndarray) and f.dtype == np.uint8 and f.ndim == 3 and f.shape[2] == 3):
                raise ValueError("a host frame must be a uint8 [h,w,3] array")
            src_at.append(at)
            pitches.append(int(f.shape[1]) * 3)
            at = _align(at + f.size)
    upload = at
    len_at = at
    at = _align(at + 4 * n)
    out_at, caps, ws_at, ws_total = [], [], [], 0
    for f, sub in zip(frames, subs):
        h, w = int(f.shape[0]), int(f.shape[1])
        cap, ws = lib.hh_jpeg_bound(h, w, sub), lib.hh_jpeg_workspace_bytes(h, w, sub)
        if cap < 0 or ws < 0:
            _lib.check(1)  # (refused by name: the size or the subsampling)
        out_at.append(at)
        caps.append(int(cap) if capacity is None else int(capacity))
        at = _align(at + caps[-1])
        ws_at.append(ws_total)
        ws_total += int(ws)
    host = torch.empty(upload, dtype=torch.uint8).pin_memory()
    hv = host.numpy()
    descs = hv[:DESC.itemsize * n].view(DESC)
    buf = torch.empty(at, dtype=torch.uint8, device=device)  # [descriptors | uploaded frames | lengths | streams, each with its bound of room]
    work = torch.empty(max(ws_total, 16), dtype=torch.uint8, device=device)
    # offsets are counted from the lowest address involved, so that none is negative (the base itself is never dereferenced)
    base = min([buf.data_ptr()] + [f.data_ptr() for f, dev in zip(frames, on_dev) if dev])
    rel = buf.data_ptr() - base
    for j, f in enumerate(frames):
        if on_dev[j]:
            src = f.data_ptr() - base
        else:
            np.copyto(hv[src_at[j]:src_at[j] + f.size].reshape(f.shape), f)
            src = rel + src_at[j]
        descs[j] = (src, rel + out_at[j], caps[j], ws_at[j], pitches[j], f.shape[0], f.shape[1], int(quals[j]), subs[j], FLAG_BGR if bgrs[j] else 0, 0)
    buf[:upload].copy_(host, non_blocking=True)
    _lib.launch(device, lib.hh_jpeg_encode_u8_batch, base, buf.data_ptr(), descs.ctypes.data, n, work.data_ptr(), work.numel(), buf.data_ptr() + len_at)
    stream = torch.cuda.current_stream(device)
    lengths_host = torch.empty(n, dtype=torch.int32, pin_memory=True)
    lengths_host.copy_(buf[len_at:len_at + 4 * n].view(torch.int32), non_blocking=True)
    stream.synchronize()
    lengths = [int(v) for v in lengths_host.numpy()]
    if any(not 0 < ln <= cap for ln, cap in zip(lengths, caps)):
        raise _lib.HHError("hh_jpeg_encode_u8_batch: a stream's length lies outside its bound")
    packed = torch.cat([buf[o:o + ln] for o, ln in zip(out_at, lengths)]) if n > 1 else buf[out_at[0]:out_at[0] + lengths[0]]
    out_host = torch.empty(sum(lengths), dtype=torch.uint8, pin_memory=True)
    out_host.copy_(packed, non_blocking=True)
    stream.synchronize()
    data = out_host.numpy().tobytes()
    ends = np.cumsum([0] + lengths)
    return [data[int(ends[j]):int(ends[j + 1])] for j in range(n)]


def save_jpeg(path, image, quality: int = 90, subsampling="420", bgr: bool = False) -> int:
    """`cv2.imwrite(path, image)` for a .jpg: the image (device tensor or numpy array, uint8 [h,w,3]) encoded on the GPU -> bytes written."""
    data = encode_jpeg_device([image], quality, subsampling, bgr)[0]
    with open(path, "wb") as f:
        f.write(data)
    return len(data)


class MJPEGWriter:
    """`cv2.VideoWriter(path, VideoWriter_fourcc(*"MJPG"), fps, (width, height))` as far as the file goes: a RIFF AVI whose frames are the
    JPEG streams handed to `write`.  Layout: RIFF 'AVI ' { LIST 'hdrl' { 'avih' (56 bytes), LIST 'strl' { 'strh' (56 bytes: 'vids', 'MJPG',
    scale 1, rate fps), 'strf' (40-byte BITMAPINFOHEADER, 24 bit, compression 'MJPG') } }, LIST 'movi' { '00dc' chunks, padded to even
    length }, 'idx1' (16-byte entries: '00dc', flags 0x10, offset from the 'movi' fourcc, size) }.  Sizes and frame counts are patched on
    close().  A file that would pass 4 GB is refused (RIFF sizes are 32 bit).  Parity with cv2's own writer and with players is UNPINNED:
    neither is available where this is tested; the tests walk the RIFF structure and decode every frame."""

    LIMIT = (1 << 32) - 1

    def __init__(self, path, fps, width: int, height: int):
        fps = int(round(float(fps)))
        if fps < 1 or not (1 <= int(width) <= 65535 and 1 <= int(height) <= 65535):
            raise ValueError("MJPEGWriter: need fps >= 1 and a frame size in 1..65535")
        self.fps, self.width, self.height = fps, int(width), int(height)
        self._index: list[tuple[int, int]] = []
        self._max = 0
        self._f = open(path, "wb")
        self._f.write(self._headers(0, 0, 0, 0))
        self._movi = self._f.tell() - 4  # the 'movi' fourcc: index offsets count from here
        self._pos = self._f.tell()

    def _headers(self, frames: int, riff_size: int, movi_size: int, max_bytes: int) -> bytes:
        w, h, fps = self.width, self.height, self.fps
        avih = struct.pack("<14I", 1000000 // fps, min(max_bytes * fps, self.LIMIT), 0, 0x10, frames, 0, 1, max_bytes, w, h, 0, 0, 0, 0)  # AVIF_HASINDEX
        strh = struct.pack("<4s4sIHHIIIIIIIIhhhh", b"vids", b"MJPG", 0, 0, 0, 0, 1, fps, 0, frames, max_bytes, 0xFFFFFFFF, 0, 0, 0, w, h)
        strf = struct.pack("<IiiHH4sIiiII", 40, w, h, 1, 24, b"MJPG", min(w * h * 3, self.LIMIT), 0, 0, 0, 0)
        assert len(avih) == 56 and len(strh) == 56 and len(strf) == 40
        strl = b"strl" + b"strh" + struct.pack("<I", 56) + strh + b"strf" + struct.pack("<I", 40) + strf
        hdrl = b"hdrl" + b"avih" + struct.pack("<I", 56) + avih + b"LIST" + struct.pack("<I", len(strl)) + strl
        return (b"RIFF" + struct.pack("<I", riff_size) + b"AVI " + b"LIST" + struct.pack("<I", len(hdrl)) + hdrl
                + b"LIST" + struct.pack("<I", movi_size) + b"movi")

    def write(self, jpeg_bytes: bytes) -> None:
        if self._f is None:
            raise ValueError("MJPEGWriter: the file is closed")
        data = bytes(jpeg_bytes)
        if data[:2] != b"\xff\xd8":
            raise ValueError("MJPEGWriter.write: not a JPEG stream")
        padded = len(data) + (len(data) & 1)
        # what the file would hold after this frame and close(): the chunk, one more index entry, the idx1 header
        if self._pos + 8 + padded + 8 + 16 * (len(self._index) + 1) > self.LIMIT:
            raise ValueError("MJPEGWriter: the file would pass 4 GB")
        self._index.append((self._pos - self._movi, len(data)))
        self._f.write(b"00dc" + struct.pack("<I", len(data)) + data + b"\0" * (padded - len(data)))
        self._pos += 8 + padded
        self._max = max(self._max, len(data))

    def close(self) -> None:
        if self._f is None:
            return
        f, self._f = self._f, None
        idx = b"".join(struct.pack("<4sIII", b"00dc", 0x10, off, size) for off, size in self._index)
        f.write(b"idx1" + struct.pack("<I", len(idx)) + idx)
        end = f.tell()
        f.seek(0)
        f.write(self._headers(len(self._index), end - 8, self._pos - self._movi, self._max))
        f.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False
