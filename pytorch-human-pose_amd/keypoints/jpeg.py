"""The files the reference's video and directory paths end in, without cv2: baseline JPEG encoded on the GPU from the rendered frames and
figures where they already are (hh_jpeg_encode_u8_batch: one call of three launches for a batch of mixed sizes; the rule is written at
that entry point in include/hhrnet.h), and the Motion-JPEG AVI of `cv2.VideoWriter(..., "MJPG", ...)` (src/base/datasets/video.py:93-106)
as a pure-Python RIFF writer.  Only compressed bytes cross to the host.  There is no CPU fallback: `encode_jpeg_host` is the same rule
compiled for the host, for tests.

The way back is here too: `decode_jpeg_device` / `load_jpeg` stand for the reference's `np.array(Image.open(path).convert("RGB"))`
(src/base/datasets/base.py:174,194) with Pillow's own bytes as the target (hh_jpeg_decode_u8_batch: one call of three launches for a
batch of mixed streams; the rule is written at that entry point), `JpegImage` is what `TrainInput.build` takes in place of a pixel
array, and `MJPEGReader` reads back what `MJPEGWriter` wrote.  `decode_jpeg_host` is the same rule compiled for the host, for tests.
With `windows=` / `window=` only a rectangle of each image is decoded (hh_jpeg_decode_window_u8_batch: the same bytes as those rows and
columns of the whole decode, from the segments and the byte slice that rectangle needs): what `classification.input.ClsInput` does with
a `JpegImage` sample's crop.  With `index="device"` the index of a restart-less stream is built on the GPU in front of the decode
(hh_jpeg_index_device_batch: no Huffman pass on the host; for files that are read once, as in inference and evaluation).
"""
from __future__ import annotations

import collections
import ctypes as C
import os
import struct

import numpy as np
import torch

from .. import _lib
from .._stage import Block, Layout, align, fill_frames, frames_to_host, per_frame, place_frames

# hh_jpeg_desc of include/hhrnet.h
DESC = _lib.struct_dtype("hh_jpeg_desc")
FLAG_BGR = 1


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
    quals, subs, bgrs = per_frame(quality, n), [_subsampling(s) for s in per_frame(subsampling, n)], per_frame(bgr, n)
    device = next((f.device for f in frames if isinstance(f, torch.Tensor)), None) or torch.device("cuda", torch.cuda.current_device())
    lay = Layout()  # [descriptors | uploaded frames | lengths | streams, each with its bound of room]
    lay.add(DESC.itemsize * n)
    places = place_frames(lay, frames, device, pitched=True)
    upload = lay.pad()
    len_at = lay.add(4 * n)
    out_at, caps, ws_at, ws_total = [], [], [], 0
    for f, sub in zip(frames, subs):
        h, w = int(f.shape[0]), int(f.shape[1])
        cap, ws = lib.hh_jpeg_bound(h, w, sub), lib.hh_jpeg_workspace_bytes(h, w, sub)
        if cap < 0 or ws < 0:
            _lib.check(1)  # (refused by name: the size or the subsampling)
        caps.append(int(cap) if capacity is None else int(capacity))
        out_at.append(lay.add(caps[-1]))
        ws_at.append(ws_total)
        ws_total += int(ws)
    blk = Block(upload, lay.pad(), device, [f for f, at in zip(frames, places) if at is None])
    descs = blk.host(0, n, DESC)
    work = torch.empty(max(ws_total, 16), dtype=torch.uint8, device=device)
    for j, (f, src) in enumerate(zip(frames, fill_frames(blk, frames, places))):
        pitch = int(f.shape[1]) * 3 if places[j] is not None else int(f.stride(0))
        descs[j] = (src, blk.off(out_at[j]), caps[j], ws_at[j], pitch, f.shape[0], f.shape[1], int(quals[j]), subs[j], FLAG_BGR if bgrs[j] else 0, 0)
    blk.upload()
    _lib.launch(device, lib.hh_jpeg_encode_u8_batch, blk.base, blk.addr(0), descs.ctypes.data, n, work.data_ptr(), work.numel(), blk.addr(len_at))
    lengths = [int(v) for v in frames_to_host([blk.tensor(len_at, (4 * n,))], copy=False)[0].view(np.int32)]
    if any(not 0 < ln <= cap for ln, cap in zip(lengths, caps)):
        raise _lib.HHError("hh_jpeg_encode_u8_batch: a stream's length lies outside its bound")
    packed = torch.cat([blk.tensor(o, (ln,)) for o, ln in zip(out_at, lengths)]) if n > 1 else blk.tensor(out_at[0], (lengths[0],))
    data = frames_to_host([packed], copy=False)[0].tobytes()
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


# ------------------------------------------------------------------------------------------------------------------ decoding
# hh_jpeg_stream_info, hh_jpeg_segment, hh_jpeg_dec_desc of include/hhrnet.h
INFO, SEGMENT, DEC_DESC, WINDOW, WIN_DESC, WIN_COUNTS = (_lib.struct_dtype("hh_jpeg_" + k) for k in (
    "stream_info", "segment", "dec_desc", "window", "win_desc", "window_counts"))
INDEX_COUNTS = ("rounds", "iterations", "iterations_worst", "subsequences", "blocks_decoded", "blocks_true")  # counts[6] of hh_debug_jpeg_index_sync_host
STATUS_NAMES = ("ok", "bad Huffman code", "zero run past coefficient 63", "bytes exhausted", "missing or unexpected RSTm", "bad segment")

JpegInfo = collections.namedtuple("JpegInfo", "h w components sampling restart_interval mcu_cols mcu_rows scan_offset scan_end")
# what a window decode of one image needs: the count of selected segments, the slice [first, end) of the file, the sizes of its table
# block and workspace, and what crosses the bus (slice and table block, each rounded up to 16)
WindowPlan = collections.namedtuple("WindowPlan", "window nsel slice tables_bytes ws_bytes staged_bytes")


def _window(window) -> np.ndarray:
    top, left, height, width = (int(v) for v in window)
    w = np.zeros(1, WINDOW)
    w[0] = (top, left, height, width)
    return w


def _bytes_view(data) -> np.ndarray:
    a = np.frombuffer(data, np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, dtype=np.uint8).reshape(-1)
    if a.size == 0:
        raise _lib.HHError("hh_jpeg_parse: not a JPEG stream (no SOI)")
    return a


def _parse(a: np.ndarray) -> np.ndarray:
    info = np.zeros(1, INFO)
    _lib.check(_lib.load().hh_jpeg_parse(a.ctypes.data, a.size, info.ctypes.data))
    return info


def jpeg_info(data) -> JpegInfo:
    """hh_jpeg_parse: the header of one stream; every stream the decoder does not take is refused here, by name (HHError)."""
    i = _parse(_bytes_view(data))[0]
    return JpegInfo(int(i["h"]), int(i["w"]), int(i["ncomp"]), int(i["sampling"]), int(i["restart_interval"]), int(i["mcols"]), int(i["mrows"]),
                    int(i["scan_offset"]), int(i["scan_end"]))


def _index_count(i, mps: int) -> int:
    nmcu, ri = int(i["mcols"]) * int(i["mrows"]), int(i["restart_interval"])
    if not ri:
        return -(-nmcu // mps)
    return nmcu // ri * -(-ri // mps) + -(-(nmcu % ri) // mps)


def build_jpeg_index(data, mcus_per_segment: int | None = None) -> np.ndarray:
    """hh_jpeg_index_host: one Huffman pass on the host -> the stream's segments (SEGMENT rows), an entry every `mcus_per_segment` MCUs
    (default: one MCU row; a parameter, not a measured optimum).  The pass validates the stream; one it cannot walk is refused by
    name.  A file's index does not change: build it once (JpegIndexCache) and hand it to every decode."""
    a = _bytes_view(data)
    i = _parse(a)[0]
    mps = int(i["mcols"]) if mcus_per_segment is None else int(mcus_per_segment)
    if mps < 1:
        raise ValueError("build_jpeg_index: mcus_per_segment must be at least 1")
    entries = np.zeros(_index_count(i, mps), SEGMENT)
    n = C.c_int(0)
    _lib.check(_lib.load().hh_jpeg_index_host(a.ctypes.data, a.size, mps, entries.ctypes.data, len(entries), C.byref(n)))
    return entries[:n.value]


def _segments(a: np.ndarray, info, index) -> np.ndarray:
    """The segments one decode uses: the supplied index, else the restart intervals (a byte scan), else an index built on the spot."""
    if index is not None:
        index = np.ascontiguousarray(index)
        if index.dtype != SEGMENT or index.ndim != 1 or len(index) < 1:
            raise ValueError("a JPEG index is a non-empty 1-d array of jpeg.SEGMENT rows (build_jpeg_index)")
        return index
    if int(info["restart_interval"]):
        entries = np.zeros(int(info["nseg_restart"]), SEGMENT)
        n = C.c_int(0)
        _lib.check(_lib.load().hh_jpeg_restart_segments(a.ctypes.data, a.size, entries.ctypes.data, len(entries), C.byref(n)))
        return entries[:n.value]
    return build_jpeg_index(a)


class JpegIndexCache:
    """path -> the file's index, built on first use; an entry is dropped when the file's size or mtime changes."""

    def __init__(self, mcus_per_segment: int | None = None):
        self.mcus_per_segment = mcus_per_segment
        self._entries: dict = {}

    def get(self, path, data=None) -> np.ndarray:
        st = os.stat(path)
        key = os.fspath(path)
        hit = self._entries.get(key)
        if hit is not None and hit[0] == (st.st_size, st.st_mtime_ns):
            return hit[1]
        if data is None:
            with open(path, "rb") as f:
                data = f.read()
        index = build_jpeg_index(data, self.mcus_per_segment)
        self._entries[key] = ((st.st_size, st.st_mtime_ns), index)
        return index

    def __len__(self) -> int:
        return len(self._entries)


def index_config() -> tuple[int, int, int, int]:
    """hh_jpeg_index_config: (lanes per workgroup, default subseq_bytes, minimum subseq_bytes, default mcus_per_segment) of the index
    built on the device."""
    cfg = (C.c_int * 4)()
    _lib.check(_lib.load().hh_jpeg_index_config(cfg))
    return tuple(cfg)


def index_sync_host(data, mcus_per_segment: int, subseq_bytes: int, lanes: int, capacity: int | None = None) -> tuple[np.ndarray, int, dict]:
    """hh_debug_jpeg_index_sync_host: the device index's shared code on the host with `lanes` subsequences per round -> (the entries,
    the status, the counts: rounds, iterations, iterations_worst, subsequences, blocks_decoded, blocks_true).  A stream the last walk
    cannot walk gives no entries and its status (1 bad code, 2 run past 63, 3 bytes exhausted); every other refusal raises HHError by
    name (tests, tools/jpeg_index_time.py; needs the library, no GPU)."""
    a = _bytes_view(data)
    i = _parse(a)[0]
    cap = max(_index_count(i, max(int(mcus_per_segment), 1)), 1) if capacity is None else int(capacity)
    entries = np.zeros(max(cap, 1), SEGMENT)
    n, status = C.c_int(0), C.c_int(0)
    counts = np.zeros(len(INDEX_COUNTS), np.int64)
    rc = _lib.load().hh_debug_jpeg_index_sync_host(a.ctypes.data, a.size, int(mcus_per_segment), int(subseq_bytes), int(lanes), entries.ctypes.data, cap,
                                                   C.byref(n), C.byref(status), counts.ctypes.data)
    if rc and not status.value:
        _lib.check(rc)
    return entries[:n.value], status.value, dict(zip(INDEX_COUNTS, (int(v) for v in counts)))


class JpegImage:
    """A compressed image where `TrainInput.build` takes a pixel array: the stream's bytes with `.h`, `.w`, `.shape`, `.dtype` and `.ndim`
    of the uint8 [h,w,3] array it decodes to.  The header is parsed here (a stream the decoder does not take is refused by name), the
    segments are the supplied `index`, else the stream's restart intervals, else an index built (and so validated) here.
    `index="device"`: no Huffman pass on the host; the entries (one every `mcus_per_segment` MCUs, default index_config()[3]) are filled
    on the GPU by hh_jpeg_index_device_batch in front of the decode (`decode_jpeg_device`, `InferenceKeypointsModel.infer_images`).
    `.segments` is None and `.device_index` True.  A stream with DRI given index="device" silently keeps its restart segments (a byte
    scan, no Huffman work either; `.device_index` is False).  A device-indexed image has no offsets on the host: a window decode,
    `TrainInput.build` and `ClsInput.build` refuse it by name (their files come back every epoch: JpegIndexCache)."""

    dtype = np.dtype(np.uint8)
    ndim = 3

    def __init__(self, data, index=None, mcus_per_segment: int | None = None):
        self.data = _bytes_view(data)
        self.info = _parse(self.data)
        self.device_index = False
        self.mcus_per_segment = None
        if isinstance(index, str):
            if index != "device":
                raise ValueError(f"JpegImage: index {index!r} is not 'device', None or a build_jpeg_index result")
            mps = index_config()[3] if mcus_per_segment is None else int(mcus_per_segment)
            if mps < 1:
                raise ValueError("JpegImage: mcus_per_segment must be at least 1")
            index = None
            if not int(self.info[0]["restart_interval"]):
                self.device_index, self.mcus_per_segment = True, mps
                self.info["reserved"][0][1] = 1  # (what hh_jpeg_index_tables writes: the device is to fill the entries)
        elif mcus_per_segment is not None:
            raise ValueError("JpegImage: mcus_per_segment belongs to index='device' (a host index is cut by build_jpeg_index)")
        self.segments = None if self.device_index else _segments(self.data, self.info[0], index)
        self.nseg = _index_count(self.info[0], self.mcus_per_segment) if self.device_index else len(self.segments)
        self.h, self.w = int(self.info[0]["h"]), int(self.info[0]["w"])
        self.shape = (self.h, self.w, 3)
        lib = _lib.load()
        self.ws_bytes = int(lib.hh_jpeg_decode_workspace_bytes(self.info.ctypes.data))
        self.tables_bytes = int(lib.hh_jpeg_decode_tables_bytes(self.info.ctypes.data, self.nseg))
        if self.ws_bytes < 0 or self.tables_bytes < 0:
            _lib.check(1)

    def staged_bytes(self) -> int:
        """What crosses the bus for this image: the stream and its table block, each rounded up to 16."""
        return align(self.data.size, 16) + align(self.tables_bytes, 16)

    def stage(self, hview: np.ndarray, at: int) -> tuple[int, int]:
        """Stream and table block into the staging bytes at `at` (a multiple of 16) -> (stream offset, tables offset).  A device-indexed
        image's block comes from hh_jpeg_index_tables: its entries are blank but for first_mcu / mcu_count."""
        tables_at = at + align(self.data.size, 16)
        hview[at:at + self.data.size] = self.data
        out = hview[tables_at:tables_at + self.tables_bytes]
        if self.device_index:
            n = C.c_int(0)
            _lib.check(_lib.load().hh_jpeg_index_tables(self.data.ctypes.data, self.data.size, self.mcus_per_segment, out.ctypes.data, self.tables_bytes,
                                                        C.byref(n)))
            return at, tables_at
        _lib.check(_lib.load().hh_jpeg_decode_tables(self.data.ctypes.data, self.data.size, self.segments.ctypes.data, len(self.segments),
                                                     out.ctypes.data, self.tables_bytes))
        return at, tables_at

    def window_plan(self, window) -> WindowPlan:
        """hh_jpeg_decode_window_select for (top, left, height, width): the segments with an MCU in the window's MCU rectangle, the byte
        slice they need, the table block's and the workspace's size.  A window that is empty or leaves the image is refused by name."""
        if self.device_index:
            raise ValueError("a window decode needs the segments' offsets on the host: a device-indexed JpegImage (index='device') has none")
        lib = _lib.load()
        w = _window(window)
        nsel, sl = C.c_int(0), (C.c_longlong * 2)()
        _lib.check(lib.hh_jpeg_decode_window_select(self.info.ctypes.data, self.segments.ctypes.data, len(self.segments), w.ctypes.data, C.byref(nsel), sl))
        tables = int(lib.hh_jpeg_decode_tables_bytes(self.info.ctypes.data, nsel.value))
        ws = int(lib.hh_jpeg_decode_window_workspace_bytes(self.info.ctypes.data, w.ctypes.data))
        if tables < 0 or ws < 0:
            _lib.check(1)
        return WindowPlan(tuple(int(v) for v in w[0]), nsel.value, (int(sl[0]), int(sl[1])), tables, ws, align(int(sl[1] - sl[0]), 16) + align(tables, 16))

    def stage_window(self, hview: np.ndarray, at: int, window, plan: WindowPlan | None = None) -> tuple[int, int, WindowPlan, np.ndarray]:
        """The window's slice of the stream and its table block (selected segments only, offsets rebased to the slice) into the staging
        bytes at `at` (a multiple of 16) -> (slice offset, tables offset, the plan, the rebased info the block starts with).  `plan`: this window's
        `window_plan`, where the caller has it already."""
        plan = self.window_plan(window) if plan is None else plan
        first, end = plan.slice
        tables_at = at + align(end - first, 16)
        hview[at:at + end - first] = self.data[first:end]
        out = hview[tables_at:tables_at + plan.tables_bytes]
        w = _window(window)
        nsel, sl = C.c_int(0), (C.c_longlong * 2)()
        _lib.check(_lib.load().hh_jpeg_decode_window_tables(self.data.ctypes.data, self.data.size, self.segments.ctypes.data, len(self.segments),
                                                            w.ctypes.data, out.ctypes.data, plan.tables_bytes, C.byref(nsel), sl))
        return at, tables_at, plan, out[:INFO.itemsize].view(INFO).copy()

    def window_desc(self, plan: WindowPlan, stream_at: int, tables_at: int, dst_at: int, ws_at: int, pitch: int, bgr: bool = False) -> tuple:
        """One WIN_DESC row for a staged window: (the DEC_DESC row `d`, the window)."""
        return ((stream_at, tables_at, plan.tables_bytes, dst_at, ws_at, pitch, plan.slice[1] - plan.slice[0], plan.nsel, FLAG_BGR if bgr else 0, 0),
                plan.window)

    def whole_plan(self) -> WindowPlan:
        """The record `window_plan` gives, for the whole-image entry: every segment, the whole stream, the MCU grid's workspace."""
        return WindowPlan((0, 0, self.h, self.w), self.nseg, (0, self.data.size), self.tables_bytes, self.ws_bytes, self.staged_bytes())

    def stage_plan(self, hview: np.ndarray, at: int, plan: WindowPlan, windowed: bool) -> tuple[int, int, np.ndarray]:
        """`stage` (a `whole_plan`) or `stage_window` -> (stream offset, tables offset, the info the library validates the image by)."""
        if not windowed:
            return (*self.stage(hview, at), self.info)
        stream_at, tables_at, _, info = self.stage_window(hview, at, plan.window, plan)
        return stream_at, tables_at, info


def launch_decode(dev, base: int, descs_dev: int, descs: np.ndarray, infos: np.ndarray, work, status_dev: int, entry: str = "hh_jpeg_decode_u8_batch") -> None:
    """`entry` on the current stream of `dev` (three launches behind the clearing of the statuses): hh_jpeg_decode_u8_batch with DEC_DESC
    rows, or hh_jpeg_decode_window_u8_batch with WIN_DESC rows and, as `infos`, the rebased infos `stage_window` returned."""
    _lib.launch(dev, getattr(_lib.load(), entry), base, descs_dev, descs.ctypes.data, infos.ctypes.data, len(descs), work.data_ptr(), work.numel(),
                status_dev)


def raise_status(statuses, what: str = "hh_jpeg_decode_u8_batch") -> None:
    bad = [(i, int(s)) for i, s in enumerate(statuses) if int(s)]
    if bad:
        i, s = bad[0]
        name = STATUS_NAMES[s] if 0 <= s < len(STATUS_NAMES) else "unknown"
        raise _lib.HHError(f"{what}: image {i}: status {s} ({name})" + (f"; also images {[j for j, _ in bad[1:]]}" if len(bad) > 1 else ""))


def launch_index(dev, base: int, descs_dev: int, descs: np.ndarray, infos: np.ndarray, mcus_per_segment: int, subseq_bytes: int | None,
                 status_dev: int) -> None:
    """hh_jpeg_index_device_batch on the current stream of `dev`, in front of `launch_decode` with the same rows: one launch behind the
    clearing of its own statuses; it fills the entries of the device-indexed images' table blocks and skips the others."""
    sub = index_config()[1] if subseq_bytes is None else int(subseq_bytes)
    _lib.launch(dev, _lib.load().hh_jpeg_index_device_batch, base, descs_dev, descs.ctypes.data, infos.ctypes.data, len(descs), int(mcus_per_segment), sub,
                None, 0, status_dev)


def index_mcus_per_segment(items: list, what: str):
    """The one mcus_per_segment of the device-indexed images of a batch (one index call serves them all), or None without any."""
    sizes = {it.mcus_per_segment for it in items if it.device_index}
    if len(sizes) > 1:
        raise ValueError(f"{what}: the device-indexed images of one batch must share one mcus_per_segment, got {sorted(sizes)}")
    return next(iter(sizes), None)


class JpegBatch:
    """The JpegImage inputs of one staged batch (`infer_images`, `TrainInput.build`, `ClsInput.build`): where their bytes lie in the
    caller's one copy, where their pixels are formed on the device, the descriptor rows, the calls.  `plans`: one `window_plan` per
    item for a window decode (WIN_DESC rows, hh_jpeg_decode_window_u8_batch); None decodes every image whole (DEC_DESC rows,
    hh_jpeg_decode_u8_batch, with ONE hh_jpeg_index_device_batch in front where an item's index is the device's to build).  In order:
    `place_upload` with the caller's Layout at the end of its uploaded bytes, `place_device` with it in the device-only tail, `fill`
    on the pinned bytes, `launch` on the device buffer.  Without items every step does nothing: the caller's layout is unchanged."""

    def __init__(self, items: list, plans: list | None = None, what: str = "JpegBatch"):
        self.items, self.windowed = list(items), plans is not None
        self.plans = list(plans) if self.windowed else [it.whole_plan() for it in self.items]
        self.desc_t = WIN_DESC if self.windowed else DEC_DESC
        self.index_mps = index_mcus_per_segment(self.items, what)
        self.calls = 2 if self.index_mps is not None else 1  # (each call has statuses of its own: the decode's, then the index call's)
        self.ws_at = np.cumsum([0] + [p.ws_bytes for p in self.plans])
        self.pixel_at: list = []

    def __len__(self) -> int:
        return len(self.items)

    def place_upload(self, lay: Layout) -> None:
        """[descriptors | stream or slice, table block | ...], each 16-aligned (`staged_bytes` is a multiple of 16: back to back)."""
        if self.items:
            self.desc_at = lay.add(self.desc_t.itemsize * len(self), 16)
            self.places = [lay.add(p.staged_bytes, 16) for p in self.plans]

    def place_device(self, lay: Layout) -> None:
        """[statuses, int32 per item and call | pixel slots, 16-aligned]: nothing of them is copied.  `pixel_at`: per item its slot."""
        if self.items:
            self.status_at = lay.add(4 * len(self) * self.calls, 4)
            self.pixel_at = [lay.add(p.window[2] * p.window[3] * 3, 16) for p in self.plans]

    def fill(self, hview: np.ndarray) -> None:
        """Streams, table blocks and descriptor rows into the pinned bytes; the infos the library validates the rows by are kept."""
        if not self.items:
            return
        self.descs = hview[self.desc_at:self.desc_at + self.desc_t.itemsize * len(self)].view(self.desc_t)
        infos = []
        for k, (it, p) in enumerate(zip(self.items, self.plans)):
            stream_at, tables_at, info = it.stage_plan(hview, self.places[k], p, self.windowed)
            infos.append(info)
            row = it.window_desc(p, stream_at, tables_at, self.pixel_at[k], int(self.ws_at[k]), 3 * p.window[3])
            self.descs[k] = row if self.windowed else row[0]  # (DEC_DESC: no window)
        self.infos = np.concatenate(infos)

    def launch(self, raw):
        """The calls on the current stream, on `raw`, the device buffer whose first bytes are the filled ones -> the int32 view of the
        statuses ([calls * n]; `codes` reduces a host copy), or None without items.  Nothing synchronises."""
        if not self.items:
            return None
        base = raw.data_ptr()
        work = torch.empty(max(int(self.ws_at[-1]), 16), dtype=torch.uint8, device=raw.device)
        if self.index_mps is not None:
            launch_index(raw.device, base, base + self.desc_at, self.descs, self.infos, self.index_mps, None, base + self.status_at + 4 * len(self))
        launch_decode(raw.device, base, base + self.desc_at, self.descs, self.infos, work, base + self.status_at,
                      "hh_jpeg_decode_window_u8_batch" if self.windowed else "hh_jpeg_decode_u8_batch")
        return raw[self.status_at:self.status_at + 4 * len(self) * self.calls].view(torch.int32)

    def codes(self, status: np.ndarray) -> np.ndarray:
        """Per item the larger of the calls' codes."""
        return np.asarray(status).reshape(self.calls, len(self)).max(axis=0)


def decode_jpeg_device(streams: list, index=None, bgr=False, device=None, out=None, windows=None, mcus_per_segment: int | None = None,
                       subseq_bytes: int | None = None, entries_out: list | None = None) -> list:
    """One hh_jpeg_decode_u8_batch, on the current stream, for a batch of JPEG streams (bytes, uint8 arrays or JpegImage) of mixed sizes,
    samplings and tables -> one uint8 [h,w,3] device tensor per stream, R,G,B or (`bgr`: one value or one per stream) B,G,R.  `index`:
    None, or one entry per stream (None or a build_jpeg_index result); a stream without DRI and without an index has its index built
    on the spot.  Bytes, tables and descriptors travel in one pinned copy; then one read of the n statuses: a nonzero one raises
    HHError naming the image and the code.  `out`: optional destinations, one uint8 [h,w,3] device tensor (or row-pitched view) per
    stream, written in place of fresh tensors.  `decode_jpeg_device.last_status` / `.last_h2d_bytes` keep the statuses and the uploaded
    bytes of the last call (the statuses also when it raises).
    `windows`: None, or one entry per stream, (top, left, height, width) or None (the whole image).  With any window given the call is
    ONE hh_jpeg_decode_window_u8_batch: only the segments that hold an MCU of a window's MCU rectangle and the byte slice they need
    cross the bus, only the window is turned into pixels, and that stream's tensor (and `out` entry) is [height, width, 3].
    `index="device"` (or "device" as a stream's entry of the list): the stream's index is built on the GPU, with no Huffman pass on the
    host: ONE hh_jpeg_index_device_batch in front of the decode call, on the same stream with the same descriptors, fills the entries
    (one every `mcus_per_segment` MCUs, default index_config()[3]; subsequences of `subseq_bytes`, default index_config()[1]) of
    the images that need it; host-indexed, DRI (which keep their restart segments) and device-indexed streams mix freely.
    `last_status` is then the larger of the two calls' codes per image.  A window of a device-indexed stream is refused by name
    (ValueError): selecting its segments needs the offsets on the host.  `entries_out`: a list that receives, per stream, the SEGMENT
    rows of its table block as the device holds them after the call (one more device-to-host copy; tests and tools)."""
    n = len(streams)
    if n == 0:
        return []
    if windows is not None and len(windows) != n:
        raise ValueError("decode_jpeg_device: `windows` has one entry per stream")
    windowed = windows is not None and any(w is not None for w in windows)
    desc_t, entry = (WIN_DESC, "hh_jpeg_decode_window_u8_batch") if windowed else (DEC_DESC, "hh_jpeg_decode_u8_batch")
    idx = per_frame(index, n) if isinstance(index, (list, tuple)) else [index] * n
    if index is not None and not isinstance(index, (list, tuple, str)) and n != 1:
        raise ValueError("decode_jpeg_device: `index` is a list with one entry per stream")
    items = [s if isinstance(s, JpegImage) else JpegImage(s, i, mcus_per_segment if isinstance(i, str) else None) for s, i in zip(streams, idx)]
    index_mps = index_mcus_per_segment(items, "decode_jpeg_device")
    if windowed and index_mps is not None:
        raise ValueError("decode_jpeg_device: a window decode needs the segments' offsets on the host: `windows` with a device-indexed stream "
                         "(index='device') is refused")
    # one plan per stream: without any window the whole stream and every segment, else the slice and the segments of its window
    plans = [it.window_plan((0, 0, it.h, it.w) if w is None else w) for it, w in zip(items, windows)] if windowed else [it.whole_plan() for it in items]
    bgrs = per_frame(bgr, n)
    device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    lay = Layout()  # [descriptors | streams or slices, and tables | statuses | pixels], 16-aligned
    lay.add(desc_t.itemsize * n, 16)
    places = [lay.add(p.staged_bytes, 16) for p in plans]  # (back to back: a multiple of 16 each)
    upload = lay.end
    status_at = lay.add(4 * n * 2, 16)  # (the decode's statuses, then the index call's)
    dst_at = [lay.add(p.window[2] * p.window[3] * 3 if out is None else 0, 16) for p in plans]
    ws_at = np.cumsum([0] + [p.ws_bytes for p in plans])
    work = torch.empty(max(int(ws_at[-1]), 16), dtype=torch.uint8, device=device)
    if out is not None:
        if len(out) != n:
            raise ValueError("decode_jpeg_device: one destination per stream")
        for o, p in zip(out, plans):
            if not (isinstance(o, torch.Tensor) and o.dtype == torch.uint8 and tuple(o.shape) == (p.window[2], p.window[3], 3) and o.device == work.device
                    and o.stride(2) == 1 and o.stride(1) == 3):
                raise ValueError("a destination must be a uint8 [height,width,3] device tensor (or a row-pitched view of one) of the stream's or its window's size")
    blk = Block(upload, lay.end, device, out or (), zero=True)
    descs = blk.host(0, n, desc_t)
    infos, tables_places = [], []
    for j, (it, p) in enumerate(zip(items, plans)):
        stream_at, tables_at, info = it.stage_plan(blk.bytes, places[j], p, windowed)
        infos.append(info)
        tables_places.append(tables_at)
        dst = blk.off(dst_at[j]) if out is None else blk.off_of(out[j])
        pitch = 3 * p.window[3] if out is None else int(out[j].stride(0))
        row = it.window_desc(p, blk.off(stream_at), blk.off(tables_at), dst, int(ws_at[j]), pitch, bgrs[j])
        descs[j] = row if windowed else row[0]  # (DEC_DESC: no window)
    blk.upload()
    infos = np.concatenate(infos)
    ncalls = 1
    if index_mps is not None:
        launch_index(device, blk.base, blk.addr(0), descs, infos, index_mps, subseq_bytes, blk.addr(status_at + 4 * n))
        ncalls = 2
    launch_decode(device, blk.base, blk.addr(0), descs, infos, work, blk.addr(status_at), entry)
    status_host = torch.empty(n * ncalls, dtype=torch.int32, pin_memory=True)
    status_host.copy_(blk.tensor(status_at, (4 * n * ncalls,)).view(torch.int32), non_blocking=True)
    if entries_out is not None:
        spans = [(rel_at + it.tables_bytes - SEGMENT.itemsize * p.nsel, SEGMENT.itemsize * p.nsel) for rel_at, it, p in zip(tables_places, items, plans)]
        packed = torch.cat([blk.tensor(o, (ln,)) for o, ln in spans]).cpu().numpy() if not windowed else None
    torch.cuda.current_stream(device).synchronize()
    statuses = status_host.numpy().reshape(ncalls, n).max(axis=0)
    decode_jpeg_device.last_h2d_bytes, decode_jpeg_device.last_status = upload, statuses.copy()
    if entries_out is not None and packed is not None:
        ends = np.cumsum([0] + [ln for _, ln in spans])
        entries_out[:] = [packed[int(ends[j]):int(ends[j + 1])].view(SEGMENT).copy() for j in range(n)]
    raise_status(statuses, "hh_jpeg_index_device_batch + " + entry if index_mps is not None else entry)
    if out is not None:
        return list(out)
    return [blk.tensor(o, (p.window[2], p.window[3], 3)) for o, p in zip(dst_at, plans)]


def decode_jpeg_host(data, bgr: bool = False, index=None, pitch: int | None = None, window=None, counts: dict | None = None) -> np.ndarray:
    """hh_debug_jpeg_decode_host: one stream through the rule compiled for the host -> uint8 [h,w,3] (tests and the GPU tests' yardstick;
    needs the library, no GPU).  `index`: decode from these segments instead of the stream's own.  `window` (top, left, height, width):
    hh_debug_jpeg_decode_window_host instead -> uint8 [height,width,3]; `counts`: a dict that receives what that decode did (segments and
    MCUs walked, MCUs stored, blocks transformed, pixels written, stream bytes needed)."""
    a = _bytes_view(data)
    lib = _lib.load()
    if window is not None:
        win = _window(window)
        hh, ww = int(win[0]["height"]), int(win[0]["width"])
        cnt = np.zeros(1, WIN_COUNTS)
        entry, before, after = lib.hh_debug_jpeg_decode_window_host, (win.ctypes.data,), (cnt.ctypes.data,)
    else:
        i = _parse(a)[0]
        hh, ww = int(i["h"]), int(i["w"])
        entry, before, after = lib.hh_debug_jpeg_decode_host, (), ()
    pitch = 3 * ww if pitch is None else int(pitch)
    out = np.zeros((max(hh, 0), max(pitch, 3 * ww, 0)), np.uint8)
    status = C.c_int(0)
    seg = None if index is None else np.ascontiguousarray(index)
    _lib.check(entry(a.ctypes.data, a.size, None if seg is None else seg.ctypes.data, 0 if seg is None else len(seg), *before, FLAG_BGR if bgr else 0,
                     out.ctypes.data, pitch, C.byref(status), *after))
    if window is not None and counts is not None:
        counts.update({k: int(cnt[0][k]) for k in WIN_COUNTS.names})
    return np.ascontiguousarray(out[:, :3 * ww]).reshape(hh, ww, 3)


def load_jpeg(path, device=None, cache: JpegIndexCache | None = None, bgr: bool = False, window=None, index=None, mcus_per_segment: int | None = None):
    """`np.array(Image.open(path).convert("RGB"))` with the pixels formed on the device -> uint8 [h,w,3] device tensor.  `cache`: a
    JpegIndexCache that keeps the file's index from call to call.  `window` (top, left, height, width): only that rectangle is decoded
    -> uint8 [height,width,3].  `index="device"`: the file's index is built on the GPU in front of the decode (no Huffman pass on the
    host; for a file that is read once), one entry every `mcus_per_segment` MCUs; with it a `cache` or a `window` is refused (ValueError)."""
    with open(path, "rb") as f:
        data = f.read()
    if index is not None:
        if index != "device" or cache is not None or window is not None:
            raise ValueError("load_jpeg: `index` is None or 'device', and 'device' goes with neither a cache nor a window (they need the offsets on the host)")
        return decode_jpeg_device([data], "device", bgr, device, mcus_per_segment=mcus_per_segment)[0]
    index = None
    if cache is not None and not jpeg_info(data).restart_interval:
        index = cache.get(path, data)
    if window is not None:
        return decode_jpeg_device([data], [index], bgr, device, windows=[window])[0]
    return decode_jpeg_device([data], [index], bgr, device)[0]


class MJPEGReader:
    """The inverse of MJPEGWriter, pure Python: walks RIFF 'AVI ' -> LIST 'hdrl' ('avih', 'strh', 'strf') -> LIST 'movi' -> 'idx1' and
    hands out the frames' JPEG streams.  len(), fps, width, height, reader[i] -> bytes, iteration; read(i, n, device) decodes n frames in
    one hh_jpeg_decode_u8_batch call.  A file that is not an MJPG AVI, or whose index is cut short, is refused by name."""

    def __init__(self, path):
        with open(path, "rb") as f:
            self._data = f.read()
        d = self._data
        if len(d) < 12 or d[:4] != b"RIFF" or d[8:12] != b"AVI ":
            raise ValueError("MJPEGReader: not a RIFF AVI file")
        self.fps = self.width = self.height = None
        movi = idx = None
        handler = None
        for fourcc, at, size in self._chunks(12, len(d)):
            if fourcc == b"LIST" and d[at:at + 4] == b"hdrl":
                for f2, a2, s2 in self._chunks(at + 4, at + size):
                    if f2 == b"avih" and s2 >= 40:
                        self.width, self.height = struct.unpack_from("<II", d, a2 + 32)
                    elif f2 == b"LIST" and d[a2:a2 + 4] == b"strl":
                        for f3, a3, s3 in self._chunks(a2 + 4, a2 + s2):
                            if f3 == b"strh" and s3 >= 28 and d[a3:a3 + 4] == b"vids":
                                handler = d[a3 + 4:a3 + 8]
                                scale, rate = struct.unpack_from("<II", d, a3 + 20)
                                self.fps = rate / scale if scale else None
            elif fourcc == b"LIST" and d[at:at + 4] == b"movi":
                movi = (at, size)
            elif fourcc == b"idx1":
                idx = (at, size)
        if handler is None or movi is None or self.fps is None:
            raise ValueError("MJPEGReader: not an AVI with a video stream and a 'movi' list")
        if handler.upper() != b"MJPG":
            raise ValueError(f"MJPEGReader: not an MJPG AVI (the video stream's handler is {handler!r})")
        if self.fps == int(self.fps):
            self.fps = int(self.fps)
        if idx is None:
            raise ValueError("MJPEGReader: truncated file: no 'idx1' chunk")
        nframes_at = None
        for fourcc, at, size in self._chunks(12, len(d)):
            if fourcc == b"LIST" and d[at:at + 4] == b"hdrl":
                for f2, a2, s2 in self._chunks(at + 4, at + size):
                    if f2 == b"avih":
                        nframes_at = struct.unpack_from("<I", d, a2 + 16)[0]
        if idx[1] % 16 or idx[0] + idx[1] > len(d):
            raise ValueError("MJPEGReader: truncated 'idx1' chunk")
        self._frames = []
        for e in range(idx[1] // 16):
            cid, _, off, size = struct.unpack_from("<4sIII", d, idx[0] + 16 * e)
            if cid[2:] not in (b"dc", b"db"):
                continue
            start = movi[0] + off + 8  # offsets count from the 'movi' fourcc; 8: the chunk's own header
            if start + size > movi[0] + movi[1] or d[start - 8:start - 4] != cid or struct.unpack_from("<I", d, start - 4)[0] != size:
                raise ValueError(f"MJPEGReader: index entry {e} does not point at a frame chunk")
            self._frames.append((start, size))
        if nframes_at is not None and nframes_at != len(self._frames):
            raise ValueError(f"MJPEGReader: truncated 'idx1' chunk: {len(self._frames)} entries for {nframes_at} frames")

    def _chunks(self, at: int, end: int):
        d = self._data
        while at + 8 <= end:
            fourcc, size = d[at:at + 4], struct.unpack_from("<I", d, at + 4)[0]
            if at + 8 + size > len(d):
                raise ValueError(f"MJPEGReader: truncated file: chunk {fourcc!r} passes the end")
            yield fourcc, at + 8, size
            at += 8 + size + (size & 1)

    def __len__(self) -> int:
        return len(self._frames)

    def __getitem__(self, i: int) -> bytes:
        start, size = self._frames[i]
        return self._data[start:start + size]

    def __iter__(self):
        return (self[i] for i in range(len(self)))

    def read(self, i: int = 0, n: int | None = None, device=None, bgr: bool = False) -> list:
        """Frames i .. i + n - 1 decoded on the device in one call -> uint8 [h,w,3] tensors."""
        n = len(self) - i if n is None else n
        if i < 0 or n < 0 or i + n > len(self):
            raise IndexError("MJPEGReader.read: frames outside the file")
        return decode_jpeg_device([self[k] for k in range(i, i + n)], None, bgr, device)
