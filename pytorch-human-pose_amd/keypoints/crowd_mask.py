"""Crowd masks from COCO segmentations, without the COCO API package: `get_crowd_mask` of the reference's dataset
(`src/keypoints/datasets/coco.py:167-177`) and the loop over it in `_save_annots_to_files`.

The split (the rule is stated at hh_crowd_polygon_toggles / hh_crowd_masks_u8_batch in include/hhrnet.h):
  * host: every segment of an image -- a polygon, a box or an uncompressed run-length list -- is reduced to a *toggle list*, a strictly
    increasing list of uint32 positions in 0 .. h*w on the column-major pixel index idx = x*h + y.  Polygons go through the library's
    hh_crowd_polygon_toggles (host code, no GPU), run-lengths through numpy;
  * device: one hh_crowd_masks_u8_batch launch fills all masks of a batch: byte 0 where at least one segment covers the pixel (an odd
    number of its toggles <= idx), 255 elsewhere.  Segments combine as a union.
`CrowdSegments` is what `TrainInput.build` takes in place of a dense crowd mask: the mask is then rasterised on the device and its
bytes never cross the bus.  There is no CPU path for the fill.

Which objects contribute follows get_crowd_mask: objects with `iscrowd` truthy and objects with `num_keypoints == 0`.  A dict
segmentation is one run-length segment (`counts` as a compressed string raises ValueError: ground-truth files do not use it).  A list
of lists follows the COCO API's dispatch on the FIRST entry: if it has exactly 4 numbers every entry is a box x, y, bw, bh, read as the
polygon (x,y), (x,y+bh), (x+bw,y+bh), (x+bw,y); otherwise every entry is a polygon, and an entry with an odd count or fewer than 6
numbers raises ValueError.  Both the polygon conversion and this dispatch are restated from memory of the package's source: parity with
the package itself is UNPINNED, the header's text is the contract."""
from __future__ import annotations

import ctypes as C

import numpy as np

from .. import _lib
from .._stage import Block, Layout, frames_to_host

# hh_crowd_mask_desc / hh_crowd_seg_desc of include/hhrnet.h (24 bytes each)
MASK_DESC, SEG_DESC = _lib.struct_dtype("hh_crowd_mask_desc"), _lib.struct_dtype("hh_crowd_seg_desc")
MAX_SIDE = 16384
CHUNK_BYTES = 64 << 20  # mask bytes per launch of `crowd_masks`


def config() -> tuple[int, int, int, int]:
    """(tile rows, tile columns, threads per workgroup, per-chunk toggle capacity or 0) of the fill kernel."""
    out = (C.c_int * 4)()
    _lib.check(_lib.load().hh_crowd_mask_config(out))
    return tuple(out)


def cancel(positions) -> np.ndarray:
    """Sorted, values of even multiplicity dropped, values of odd multiplicity kept once -> uint32."""
    values, counts = np.unique(np.asarray(positions, np.int64), return_counts=True)
    return values[counts % 2 == 1].astype(np.uint32)


def rle_toggles(counts, h: int, w: int) -> np.ndarray:
    """An uncompressed COCO run-length list -> its toggle list: the cumulative sums without the last, zero-length runs cancelled."""
    if isinstance(counts, (str, bytes)):
        raise ValueError("crowd mask: compressed run-length strings are not supported")
    counts = np.asarray(counts)
    if counts.ndim != 1 or counts.size == 0 or not np.issubdtype(counts.dtype, np.integer) or (counts < 0).any():
        raise ValueError("crowd mask: run lengths must be a list of non-negative integers")
    sums = np.cumsum(counts.astype(np.int64))
    if int(sums[-1]) != h * w:
        raise ValueError(f"crowd mask: run lengths sum to {int(sums[-1])}, the image has {h * w} pixels")
    return cancel(sums[:-1])


def polygon_toggles(xy, h: int, w: int) -> np.ndarray:
    """One polygon x0, y0, x1, y1, ... -> its toggle list (hh_crowd_polygon_toggles; HHError for what that refuses)."""
    xy = np.ascontiguousarray(np.asarray(xy, np.float64).reshape(-1))
    if xy.size % 2 or xy.size < 6:
        raise ValueError("crowd mask: a polygon needs an even count of at least 6 numbers")
    lib = _lib.load()
    k = xy.size // 2
    cap = lib.hh_crowd_polygon_capacity(xy.ctypes.data, k, int(h), int(w))
    if cap < 0:
        _lib.check(1)
    out = np.empty(max(int(cap), 1), np.uint32)
    n = lib.hh_crowd_polygon_toggles(xy.ctypes.data, k, int(h), int(w), out.ctypes.data, int(cap))
    if n < 0:
        _lib.check(1)
    return out[:n].copy()


def segmentation_toggles(segmentation, h: int, w: int) -> list:
    """One object's `segmentation` -> its toggle lists, by the dispatch of the module docstring."""
    if isinstance(segmentation, dict):
        if [int(v) for v in segmentation["size"]] != [h, w]:
            raise ValueError(f"crowd mask: run-length size {segmentation['size']} differs from the image {[h, w]}")
        return [rle_toggles(segmentation["counts"], h, w)]
    entries = list(segmentation)
    if any(not isinstance(e, (list, tuple, np.ndarray)) for e in entries):
        raise ValueError("crowd mask: a segmentation is a run-length dict or a list of lists")
    if entries and len(entries[0]) == 4:
        out = []
        for e in entries:
            if len(e) != 4:
                raise ValueError("crowd mask: a box needs exactly 4 numbers")
            x, y, bw, bh = (float(v) for v in e)
            out.append(polygon_toggles([x, y, x, y + bh, x + bw, y + bh, x + bw, y], h, w))
        return out
    return [polygon_toggles(e, h, w) for e in entries]


class CrowdSegments:
    """The segments that define one image's crowd mask: `toggle_lists` is a list of strictly increasing integer sequences in
    0 .. h*w, one per segment.  `.shape == (h, w)`.  Empty lists are dropped (they cover nothing)."""

    def __init__(self, h: int, w: int, toggle_lists=()):
        self.h, self.w = int(h), int(w)
        if not (1 <= self.h <= MAX_SIDE and 1 <= self.w <= MAX_SIDE):
            raise ValueError(f"CrowdSegments: image size outside 1..{MAX_SIDE}")
        self.toggle_lists = []
        for t in toggle_lists:
            t64 = np.asarray(t, np.int64).reshape(-1)
            if t64.size == 0:
                continue
            if t64[0] < 0 or t64[-1] > self.h * self.w or (np.diff(t64) <= 0).any():
                raise ValueError("CrowdSegments: toggles must be strictly increasing in 0 .. h*w")
            self.toggle_lists.append(t64.astype(np.uint32))

    @property
    def shape(self) -> tuple[int, int]:
        return (self.h, self.w)

    @property
    def num_toggles(self) -> int:
        return sum(t.size for t in self.toggle_lists)

    @property
    def table_bytes(self) -> int:
        """What this mask adds to a batch's staged bytes: its descriptor, its segment descriptors and its toggles."""
        return MASK_DESC.itemsize + SEG_DESC.itemsize * len(self.toggle_lists) + 4 * self.num_toggles

    def column_range(self, t: np.ndarray) -> tuple[int, int]:
        """The inclusive range of columns a toggle list can cover: from the first toggle's column to the column of the pixel before
        the last toggle (through the last column for an odd count)."""
        first = min(int(t[0]) // self.h, self.w - 1)
        last = self.w - 1 if t.size & 1 else max((int(t[-1]) - 1) // self.h, first)
        return first, last

    @classmethod
    def from_annotations(cls, annot, h: int, w: int) -> "CrowdSegments":
        """The objects of get_crowd_mask (`iscrowd` truthy, or `num_keypoints == 0`), their segmentations reduced to toggle lists."""
        lists = []
        for obj in annot:
            if obj["iscrowd"] or obj["num_keypoints"] == 0:
                lists.extend(segmentation_toggles(obj["segmentation"], int(h), int(w)))
        return cls(h, w, lists)


def tables_bytes(items) -> int:
    return sum(s.table_bytes for s in items)


def fill_tables(items, mask_offsets, hview: np.ndarray, at: int) -> tuple[int, int, int]:
    """Write the tables of `items` (CrowdSegments) into the staged bytes `hview` from byte `at` (a multiple of 8) on: mask descriptors,
    segment descriptors, toggles, `tables_bytes(items)` bytes in all.  mask_offsets[i] is where mask i is to lie, in bytes from the
    buffer's start.  -> (offset of the mask descriptors, offset of the segment descriptors, number of segments)."""
    assert at % 8 == 0
    n, nseg = len(items), sum(len(s.toggle_lists) for s in items)
    seg_at = at + MASK_DESC.itemsize * n
    tog_at = seg_at + SEG_DESC.itemsize * nseg
    mdescs = hview[at:seg_at].view(MASK_DESC)
    sdescs = hview[seg_at:tog_at].view(SEG_DESC)
    s = 0
    for i, item in enumerate(items):
        mdescs[i] = (int(mask_offsets[i]), item.h, item.w, s, len(item.toggle_lists))
        for t in item.toggle_lists:
            sdescs[s] = (tog_at, t.size, *item.column_range(t), 0)
            hview[tog_at:tog_at + 4 * t.size].view(np.uint32)[:] = t
            tog_at += 4 * t.size
            s += 1
    return at, seg_at, nseg


def launch(dev, base: int, host_base: int, desc_at: int, seg_at: int, n: int, nseg: int) -> None:
    """hh_crowd_masks_u8_batch on the current stream of `dev`: the tables lie at the same offsets behind `base` (device) and
    `host_base` (the staged host copy, which is what the library validates)."""
    lib = _lib.load()
    _lib.launch(dev, lib.hh_crowd_masks_u8_batch, base, base + desc_at, base + seg_at if nseg else None, host_base + desc_at,
                host_base + seg_at if nseg else None, host_base, n, nseg)


def crowd_masks(segments, device="cuda:0") -> list:
    """[CrowdSegments] -> [bool [h,w] array], True where no segment covers the pixel (what get_crowd_mask returns).  Per chunk of at
    most CHUNK_BYTES mask bytes: one pinned copy up (tables and toggles only), one launch, one pinned copy down."""
    import torch
    segments = list(segments)
    dev = torch.device(device)
    out, first = [], 0
    while first < len(segments):
        last, nbytes = first, 0
        while last < len(segments) and (last == first or nbytes + segments[last].h * segments[last].w <= CHUNK_BYTES):
            nbytes += (segments[last].h * segments[last].w + 3) // 4 * 4  # every mask starts on a dword
            last += 1
        items = segments[first:last]
        lay = Layout()  # [tables and toggles | masks, each on a dword]
        lay.add(tables_bytes(items))
        staged = lay.pad()
        offs = [lay.add(s.h * s.w, 4) for s in items]
        with torch.cuda.device(dev):
            blk = Block(staged, lay.pad(4), dev)
            desc_at, seg_at, nseg = fill_tables(items, offs, blk.bytes, 0)
            blk.upload()
            launch(dev, blk.addr(0), blk.bytes.ctypes.data, desc_at, seg_at, len(items), nseg)
            flat = frames_to_host([blk.tensor(staged, (lay.end - staged,))], copy=False)[0]
        for s, o in zip(items, offs):
            out.append(flat[o - staged:o - staged + s.h * s.w].reshape(s.h, s.w) != 0)
        first = last
    return out


def get_crowd_mask(annot: list, img_h: int, img_w: int, device="cuda:0") -> np.ndarray:
    """The reference's get_crowd_mask (coco.py:167-177), plus `device`: bool [img_h,img_w], False on crowd / unlabelled-person pixels."""
    return crowd_masks([CrowdSegments.from_annotations(annot, img_h, img_w)], device)[0]


def raw_sample(image: np.ndarray, annot: list, num_kpts: int = 17):
    """One image and its COCO annotation -> the raw sample (image, CrowdSegments, joints [P,num_kpts,3]) that `TrainInput` takes:
    coco.py:464-465, the objects with `iscrowd == 0 or num_keypoints > 0` through get_coco_joints (:68-74)."""
    h, w = np.asarray(image).shape[:2]
    segments = CrowdSegments.from_annotations(annot, h, w)
    kept = [obj for obj in annot if obj["iscrowd"] == 0 or obj["num_keypoints"] > 0]
    joints = np.zeros((len(kept), num_kpts, 3))
    for i, obj in enumerate(kept):
        joints[i] = np.array(obj["keypoints"]).reshape([-1, 3])
    return image, segments, joints
