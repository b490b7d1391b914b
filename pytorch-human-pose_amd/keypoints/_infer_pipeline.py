"""The stages of `InferenceKeypointsModel.infer_images`, the batched path behind the reference's single-image interface (`__call__` per
image, bin/eval.py:18-49): `check_options` (what is refused before anything is enqueued), `plan_batches` (images -> jobs),
`batch_layout` (the bytes of one batch's one copy; pure arithmetic) and `Pipeline`, whose `stage`, `enqueue` and `collect` the
driver calls per batch: stage k+1, enqueue k+1, collect k.  Every option is described at the stage that implements it."""
from __future__ import annotations

import functools
import itertools
from dataclasses import dataclass
from typing import NamedTuple

import numpy as np
import torch

from .. import _lib
from .._stage import Layout, PinnedRing
from . import jpeg as jp
from . import pose_score as ps
from .results import InferenceKeypointsResult, inverse_affine, transform_coords
from .transforms_utils import IMAGENET_MEAN, IMAGENET_STD, dst_to_src_matrix, get_multi_scale_size

# byte offset of the image in the batch buffer, its size, destination -> source affine
_IMAGE_DESC = _lib.struct_dtype("hh_image_desc")
RENDER_OPTIONS = {"color_mode", "alpha", "bgr", "out_height", "jpeg", "labels"}


def check_options(render: dict | None, tracker, score: str | None, n_images: int, num_kpts: int, max_num_people: int):
    """What the launches would refuse, refused before anything is enqueued (ValueError) -> the variances `score` uses, or None.
    `render`: only the options `Pipeline._render` knows, one `labels` entry per image, color_mode "track" only with a tracker.
    `score`: None, "oks" or "pckh"; a parser that keeps more than HH_POSE_MAX_P people is refused; "oks" uses the COCO constants and
    so needs the 17 COCO keypoints, PCKh reads no variance.  (`scales` and the tracker's clip are refused by `plan_batches`.)"""
    if render is not None and render.get("color_mode") == "track" and tracker is None:
        raise ValueError("infer_images: render color_mode 'track' needs a tracker")
    if render is not None:
        unknown = set(render) - RENDER_OPTIONS
        if unknown:
            raise ValueError(f"infer_images: unknown render option(s) {sorted(unknown)}")
        if render.get("labels") is not None and len(render["labels"]) != n_images:
            raise ValueError("infer_images: render labels: one list of strings (or None) per image")
    if score not in (None, "oks", "pckh"):
        raise ValueError(f"infer_images: score must be None, 'oks' or 'pckh', got {score!r}")
    if score is None:
        return None
    if max_num_people > ps.MAX_P:
        raise ValueError(f"infer_images: score= takes at most HH_POSE_MAX_P ({ps.MAX_P}) people per image, the parser keeps {max_num_people}")
    return ps.coco_variances(num_kpts) if score == "oks" else np.ones(num_kpts)


class _Shape:
    """What get_multi_scale_size reads of an image: its shape."""

    def __init__(self, h: int, w: int):
        self.shape = (int(h), int(w))


def plan_multi_scale(shapes, input_size: int, scales, max_batch: int) -> list[dict]:
    """Host plan of the batched multi-scale test (pure arithmetic, no device): raw image shapes [(h, w), ...] -> chunks, each
    {"images": indices into `shapes`, "sizes": the (w, h) of the model input at every scale, "sub_batches": per scale the
    consecutive (lo, hi) ranges of the chunk that run as one forward}; all three follow the order of `scales`, which is the
    accumulation order of `multi_scale_maps`.
    Buckets: images whose model-input sizes agree at EVERY scale (get_multi_scale_size truncates per scale, so the scale-1 size
    alone need not fix the others).  Chunks: at most `max_batch` images of a bucket.  Sub-batches at scale s: n_s =
    min(len(chunk), max(1, max_batch * h_1*w_1 // (h_s*w_s))) images, so that no forward carries more input pixels than the
    scale-1 forward of `max_batch` images that the single-scale path runs."""
    scales = tuple(scales)
    if 1.0 not in scales:
        raise ValueError("plan_multi_scale: scales must contain 1.0 (the scale-1 pass provides the tags and the output geometry)")
    if max_batch < 1:
        raise ValueError("plan_multi_scale: max_batch must be >= 1")
    mn = min(scales)
    buckets: dict[tuple, list[int]] = {}
    for i, (h, w) in enumerate(shapes):
        key = tuple(tuple(get_multi_scale_size(_Shape(h, w), input_size, s, mn)[0]) for s in scales)
        buckets.setdefault(key, []).append(i)
    plan = []
    for sizes, idxs in buckets.items():
        w1, h1 = sizes[scales.index(1.0)]
        for lo in range(0, len(idxs), max_batch):
            chunk = idxs[lo:lo + max_batch]
            subs = []
            for (ws, hs) in sizes:
                n_s = min(len(chunk), max(1, max_batch * h1 * w1 // (hs * ws)))
                subs.append([(a, min(a + n_s, len(chunk))) for a in range(0, len(chunk), n_s)])
            plan.append({"images": chunk, "sizes": sizes, "sub_batches": subs})
    return plan


class Plan(NamedTuple):
    scales: tuple     # the scales every image runs at; (1,) without `scales`
    min_scale: float
    i1: int           # where scale 1 is among them: its pass gives the tags, the output geometry and the un-warp
    geo: list         # per image (size, center, scale) of its scale-1 model input
    jobs: list        # [(sizes: the (w, h) of the model input per scale, chunk: image indices, sub_batches per scale or None)]


def plan_batches(images: list, input_size: int, scales, max_batch: int, tracker=None) -> Plan:
    """Images -> the batches that run.  Without `scales` the images are bucketed by model-input shape and every bucket runs as batches of
    up to `max_batch`.  `scales` = tuple of scales: the multi-scale test of `call_multi_scale(image, annot, scales)` for every image,
    batched the same way (plan_multi_scale: buckets by the sizes at every scale, chunks of up to `max_batch`).  Bucketing reads `.shape`.
    `tracker` = a keypoints.tracking.PoseTracker with one stream: the images are consecutive frames of ONE clip.  All must share one
    model-input shape (else ValueError, before any launch) and that of the frames the tracker saw before (else reset() it)."""
    # (size, center, scale) now -- the bucket key --, the warp matrix when the image's batch is staged: the first batch should not
    # wait for n matrix inversions
    if scales is None:
        pass_scales, mn = (1,), 1
        geo = [get_multi_scale_size(img, input_size, 1, 1) for img in images]
        buckets: dict[tuple, list[int]] = {}
        for i, g in enumerate(geo):
            buckets.setdefault(tuple(g[0]), []).append(i)
        jobs = [((size,), idxs[lo:lo + max_batch], None) for size, idxs in buckets.items() for lo in range(0, len(idxs), max_batch)]
    else:
        pass_scales = tuple(scales)
        jobs = [(c["sizes"], c["images"], c["sub_batches"]) for c in plan_multi_scale([img.shape[:2] for img in images], input_size, pass_scales, max_batch)]
        mn = min(pass_scales)
        geo = [get_multi_scale_size(img, input_size, 1.0, mn) for img in images]  # the un-warp is the scale-1 pass's
    i1 = pass_scales.index(1)
    if tracker is not None and images:
        if tracker.streams != 1:
            raise ValueError("infer_images: the tracker must have one stream (the images are one clip)")
        shapes = {tuple(sizes[i1]) for sizes, _, _ in jobs}
        if len(shapes) != 1:
            raise ValueError(f"infer_images: the frames of a tracked clip must share one model-input shape, got (w, h) = {sorted(shapes)}")
        tracker.bind_input_shape(next(iter(shapes))[::-1])
    return Plan(pass_scales, mn, i1, geo, jobs)


class BatchLayout(NamedTuple):
    offs: np.ndarray  # [nb + 1]: image j's shipped pixels are bytes offs[j] .. offs[j+1] of the copy (none for a JpegImage)
    desc_off: int     # the hh_image_desc rows, one block of nb per scale, back to back
    scale_desc: list  # per scale the offset of its block
    jpeg_at: list     # which images of the batch are JpegImages
    jpegs: jp.JpegBatch
    upload: int       # the bytes that cross
    device_total: int  # the device buffer: the statuses and pixel slots of the JpegImages lie behind the uploaded bytes
    pixel_at: list    # per image where its pixels lie in the device buffer


def batch_layout(images: list, num_scales: int) -> BatchLayout:
    """The byte layout of one batch's one copy (no torch, no library call): [pixels | image descriptors, one block per scale | JPEG
    decode descriptors | streams and table blocks] on the host, [statuses | pixel slots] behind them on the device only.  `images`:
    arrays (their `.size` bytes are shipped) and JpegImages (which ship no pixels)."""
    jpeg_at = [j for j, img in enumerate(images) if isinstance(img, jp.JpegImage)]
    offs = np.cumsum([0] + [0 if isinstance(img, jp.JpegImage) else img.size for img in images])
    lay = Layout(int(offs[-1]))
    scale_desc = [lay.add(_IMAGE_DESC.itemsize * len(images)) for _ in range(num_scales)]  # (64-byte rows: the blocks stay back to back)
    jpegs = jp.JpegBatch([images[j] for j in jpeg_at], what="infer_images")
    jpegs.place_upload(lay)
    upload = lay.end
    jpegs.place_device(lay)
    pixel_at = [int(o) for o in offs[:-1]]
    for j, at in zip(jpeg_at, jpegs.pixel_at):
        pixel_at[j] = at
    return BatchLayout(offs, scale_desc[0], scale_desc, jpeg_at, jpegs, upload, lay.end, pixel_at)


class Staged(NamedTuple):
    """One batch in its pinned buffer, nothing enqueued yet."""
    chunk: list
    sizes: tuple
    subs: list | None
    layout: BatchLayout
    turn: int          # the pipeline slot: picks the staging buffer, the _score_stage buffer and the _out_ring buffers
    host: torch.Tensor
    targets: tuple | None  # (packed targets, inverse resize matrices) of a scored batch with an annotation


@dataclass
class HandOver:
    """The pinned host copies of what one batch sends back, by name; each a tuple of tensors, None where the batch has no such part."""
    decode: tuple
    track: tuple | None = None        # (ids, smoothed coordinates)
    score: tuple | None = None        # (the score blob,)
    jpeg_status: tuple | None = None  # (the decode's statuses, then the index call's where it ran,)


@dataclass
class Batch:
    """One enqueued batch: what `collect` needs once `done` has passed."""
    staged: Staged
    x: torch.Tensor
    hms: list
    tags: list
    host: HandOver
    done: torch.cuda.Event
    raw: torch.Tensor  # the batch's device bytes, alive until its render has run
    scored: ps.DeviceScore | None


class Pipeline:
    """One `infer_images` call.  Two-deep software pipeline: while the GPU works on batch k the host stages the pixels of batch k+1 into
    a pinned buffer and only then collects the results of batch k (two staging buffers, each guarded by the event of its last use)."""

    def __init__(self, model, plan: Plan, images: list, annots: list, render: dict | None, tracker, score: str | None, score_vars):
        self.model, self.plan, self.images, self.annots = model, plan, images, annots
        self.render, self.tracker, self.score, self.score_vars = render, tracker, score, score_vars
        self.results: list = [None] * len(images)
        self.staging = PinnedRing()
        self.mean, self.std = IMAGENET_MEAN.ctypes.data, IMAGENET_STD.ctypes.data

    def stage(self, sizes: tuple, chunk: list, subs) -> Staged:
        """ONE pinned buffer per batch: the raw uint8 pixels, behind them one hh_image_desc block per scale, behind those what the
        JpegImages of the batch ship.  An entry of the images may be a `jpeg.JpegImage` (bytes were made one by the driver), mixed
        freely with arrays: the stream and table block of such an image travel in the same copy, its pixel slot lies behind the
        uploaded bytes in the same device buffer.  `model.last_h2d_bytes` gains the bytes that cross.
        `score`: the annotations are packed (and refused, if they must be) before anything of this batch is enqueued; a batch without
        any annot packs nothing."""
        m, plan = self.model, self.plan
        imgs = [self.images[i] for i in chunk]
        lay = batch_layout(imgs, len(sizes))
        targets = None
        if self.score is not None and any(self.annots[i] is not None for i in chunk):
            targets = (ps.pack_targets([self.annots[i] for i in chunk], self.score, num_kpts=m._parser.num_kpts),
                       np.stack([inverse_affine(plan.geo[i][1], plan.geo[i][2], sizes[plan.i1]) for i in chunk]))
        m.last_h2d_bytes += lay.upload
        turn, host = self.staging.take(lay.upload)
        hview = host.numpy()
        nb = len(chunk)
        descs = hview[lay.desc_off:lay.desc_off + _IMAGE_DESC.itemsize * nb * len(sizes)].view(_IMAGE_DESC)
        for j, (i, img) in enumerate(zip(chunk, imgs)):
            if not isinstance(img, jp.JpegImage):
                np.copyto(hview[lay.offs[j]:lay.offs[j + 1]].reshape(img.shape), img, casting="same_kind")
            for si, s in enumerate(plan.scales):
                g = plan.geo[i] if si == plan.i1 else get_multi_scale_size(img, m.input_size, s, plan.min_scale)
                descs[si * nb + j] = (lay.pixel_at[j], img.shape[0], img.shape[1], dst_to_src_matrix(g[1], g[2], g[0]).reshape(6))
        lay.jpegs.fill(hview)
        return Staged(chunk, sizes, subs, lay, turn, host, targets)

    def enqueue(self, st: Staged) -> Batch:
        """ONE host->device copy, on a copy stream of its own, so that the pixels of this batch cross PCIe while the previous batch still
        computes (25 MB per batch of 32 512x512 images: ~1.7 ms that would otherwise sit on the compute stream); then `_launch` on the
        model's high-priority stream, for batches as for single images (same-box alternation with the caller's stream,
        tools/api_throughput.py: 3820 / 3380 against 2600 / 2970 img/s)."""
        m, lay = self.model, st.layout
        if m._copy_stream is None:
            m._copy_stream = torch.cuda.Stream(m.device)
            # (the priority of the compute stream: at a lower one the result copies would wait for the whole next batch)
            m._d2h_stream = torch.cuda.Stream(m.device, priority=torch.cuda.Stream.priority_range()[1])
        with torch.cuda.stream(m._copy_stream):
            if not lay.jpeg_at:
                raw = st.host[:lay.upload].to(m.device, non_blocking=True)
            else:  # (room behind the uploaded bytes for the statuses and the decoded pixels)
                raw = torch.empty(lay.device_total, dtype=torch.uint8, device=m.device)
                raw[:lay.upload].copy_(st.host[:lay.upload], non_blocking=True)
            copied = torch.cuda.Event()
            copied.record()
        batch = m._on_fast_stream(functools.partial(self._launch, st, raw, copied))
        self.staging.release(st.turn, copied)
        return batch

    def _prepare(self, st: Staged, raw: torch.Tensor, si: int) -> torch.Tensor:
        """The model inputs of the batch at scale `si`: one hh_preprocess_u8_batch for the whole batch, whatever the raw sizes."""
        m, nb, (ws, hs) = self.model, len(st.chunk), st.sizes[si]
        xs = torch.empty((nb, 3, hs, ws), device=m.device, dtype=torch.float32)
        _lib.launch(xs.device, m._lib.hh_preprocess_u8_batch, raw.data_ptr(), raw.data_ptr() + st.layout.scale_desc[si], nb, xs.data_ptr(), hs, ws,
                    self.mean, self.std)
        return xs

    def _launch(self, st: Staged, raw: torch.Tensor, copied) -> Batch:
        """The launches of one batch, on the current stream, behind its copy: hh_preprocess_u8 per image into one [B,3,h,w] tensor, one
        (flip-TTA) forward, one hh_decode, one device->host copy of the small result arrays (`_hand_over`).
        JpegImages: ONE hh_jpeg_index_device_batch (for the images whose index the device builds) and ONE hh_jpeg_decode_u8_batch fill
        the pixel slots in front of hh_preprocess_u8_batch, which reads them exactly as it reads shipped pixels, so `scales`, `render`
        and `tracker` work unchanged; the decoder's statuses ride in the hand-over.
        `scales`: the raw pixels still cross once; one hh_preprocess_u8_batch per scale, the forwards of the plan, one
        hh_multi_scale_aggregate per stage (and image range) instead of the per-scale flip merges and accumulations, one hh_decode on
        the averaged maps and the scale-1 tags.
        `tracker`: the chunks are fed in order, each as one hh_track_step behind its hh_decode on the same stream with
        frames_per_stream = the chunk length; ids and smoothed coordinates come back in the hand-over.
        `score`: ONE hh_pose_score_batch per batch behind its hh_decode (and behind the tracker's launch where there is one) on the same
        stream, reading the decode's outputs in place with the image's inverse resize matrix (the scale-1 geometry with `scales`); the
        target tables cross in one small pinned copy, the outputs ride as one more array in the hand-over.  The output array's size
        is rounded up to a power of two, so the pinned result buffers are shared by batches of different target counts.  A batch
        without any annot launches nothing."""
        m = self.model
        cur = torch.cuda.current_stream(m.device)
        cur.wait_event(copied)
        raw.record_stream(cur)
        jstatus = st.layout.jpegs.launch(raw)
        x = self._prepare(st, raw, self.plan.i1)
        if st.subs is None:
            hms, tags = m.forward_tta(x)
        else:
            hms, tags = m._multi_scale_maps_batch(self.plan.scales, st.subs, x, functools.partial(self._prepare, st, raw))
        out = {"decode": tuple(m._parser.decode_batch_device(hms[0], hms[1], tags, adjust=True, refine=True))}
        if self.tracker is not None:
            out["track"] = tuple(self.tracker.update_device(*out["decode"], frames_per_stream=len(st.chunk))[:2])
        scored = None
        if st.targets is not None:
            # (this slot's previous batch has been collected, so its table copy has finished: the pinned buffer is free)
            scored = ps.score_device(st.targets[0], decode=out["decode"][:4], inv_affine=st.targets[1], metric=self.score, variances=self.score_vars,
                                     stage=m._score_stage[st.turn])
            out["score"] = (scored.blob,)
        if jstatus is not None:
            out["jpeg_status"] = (jstatus,)
        host, done = self._hand_over(st.turn, out)
        return Batch(st, x, hms, tags, host, done, raw, scored)

    def _hand_over(self, turn: int, out: dict):
        """Device -> host of the named tuples of arrays of one batch -> (HandOver, the event behind the copies).  Into pinned buffers kept
        per pipeline slot and per shapes and dtypes (allocating pinned memory costs ~0.4 ms per array); `collect` of this slot's previous
        batch ran before this point and copied what it keeps.  On a stream of their own behind the decode, so that the next batch's
        launches do not queue behind the copies."""
        m = self.model
        flat = [t for part in out.values() for t in part]
        key = (turn, tuple((tuple(t.shape), t.dtype) for t in flat))
        if key not in m._out_ring:
            m._out_ring[key] = [torch.empty(t.shape, dtype=t.dtype, pin_memory=True) for t in flat]
        decoded = torch.cuda.Event()
        decoded.record()
        with torch.cuda.stream(m._d2h_stream):
            m._d2h_stream.wait_event(decoded)
            copies = iter([h.copy_(t, non_blocking=True) for h, t in zip(m._out_ring[key], flat)])
            done = torch.cuda.Event()
            done.record()
        for t in flat:
            t.record_stream(m._d2h_stream)
        return HandOver(**{name: tuple(itertools.islice(copies, len(part))) for name, part in out.items()}), done

    def collect(self, b: Batch) -> None:
        """Device -> host results of one enqueued batch (ONE event wait), un-warp, result objects: every image gets the result
        `model(image, annot)` returns (same kernels on the same per-image data: images of a batch are independent).
        JpegImages: a nonzero status raises HHError naming the image, here and not before.  `.raw_image` of such a result is formed on
        first access by `decode_jpeg_host` (bit-identical to the device pixels) and cached; no pixels are copied back.
        `tracker`: every result gains `.track_ids` (int32 [P], 0 = no track) and `.kpts_coords_smooth` ([P,K,2], raw-image pixels),
        aligned with its rows."""
        m, st, geo = self.model, b.staged, self.plan.geo
        w, h = size = st.sizes[self.plan.i1]
        b.done.synchronize()
        if b.host.jpeg_status is not None:
            self._raise_bad_jpeg(st, b.host.jpeg_status[0].numpy())
        lists = m._parser.to_lists(*b.host.decode)  # (copies what it returns: the pinned buffers are reused two batches later)
        m.model_input_shape = (h, w)
        for j, i in enumerate(st.chunk):
            joints, scores = lists[j]
            coords = transform_coords(joints[..., :2], geo[i][1], geo[i][2], size)
            r = self.results[i] = InferenceKeypointsResult(self.images[i], self.annots[i], b.x[j], coords, joints[..., 2], joints[..., 3:], scores,
                                                           m.det_thr, m.tag_thr, m.limbs, [t[j:j + 1] for t in b.hms], [t[j:j + 1] for t in b.tags])
            if b.host.track is not None:
                ids, smooth = b.host.track
                r.track_ids = ids[j, :len(joints)].numpy().copy()
                r.kpts_coords_smooth = transform_coords(smooth[j, :len(joints)].numpy(), geo[i][1], geo[i][2], size).astype(coords.dtype)
        if b.scored is not None:
            self._attach_scores(st.chunk, b.scored.split(b.host.score[0]), b.scored.t_off)
        if self.render is not None:
            self._render(b)

    def _raise_bad_jpeg(self, st: Staged, status: np.ndarray) -> None:
        """The decoder's statuses came with the results: the index call's codes, if it ran, behind the decode's."""
        bad = [(st.chunk[j], int(s)) for j, s in zip(st.layout.jpeg_at, st.layout.jpegs.codes(status)) if int(s)]
        if bad:
            i, s = bad[0]
            name = jp.STATUS_NAMES[s] if 0 <= s < len(jp.STATUS_NAMES) else "unknown"
            raise _lib.HHError(f"infer_images: image {i}: its JPEG stream cannot be decoded: status {s} ({name})"
                               + (f"; also images {[k for k, _ in bad[1:]]}" if len(bad) > 1 else ""))

    def _attach_scores(self, chunk: list, parts: dict, t_off) -> None:
        """`score`: every image whose annot is not None gains `.oks`, `.object_oks`, `.kpt_oks`, `.target_matches` (`.pckh`,
        `.object_pckh`, `.kpt_pckh` for "pckh", whose objects carry "head_xyxy"); a later `calculate_OKS()` returns the stored value."""
        for j, i in enumerate(chunk):
            if self.annots[i] is not None:
                a, e = int(t_off[j]), int(t_off[j + 1])
                self.results[i]._set_score(self.score, -1 if e == a else float(parts["value"][j]), parts["obj"][a:e], parts["kpt"][a:e], parts["match"][a:e])

    def _render(self, b: Batch) -> None:
        """`render` = dict(color_mode="person", alpha=0.8, bgr=False, out_height=None): every result also carries `.rendered`, the overlay
        frame of `result.plot_connections(color_mode, alpha)` (B,G,R order if `bgr`; resized to `out_height` with the aspect ratio kept,
        as the reference's resize_with_aspect_ratio, if given).  The frames of a batch are drawn in ONE hh_render_poses_u8_batch from the
        staged device pixels of that batch, which stay alive until then (`model._render_chunk`).  With `jpeg=dict(quality=90,
        subsampling="420")` among the options the frames of a batch are encoded on the GPU in ONE hh_jpeg_encode_u8_batch behind their
        render launch (keypoints/jpeg.py) and every result carries `.rendered_jpeg` (bytes; true colours also with `bgr`) in place of
        `.rendered`: no raw frame is copied back.  color_mode="track" (needs `tracker`) draws the smoothed coordinates, each person in
        the colour of its id.  With `labels=[[str, ...] or None, ...]` among the options, one list per image of the call, every finished
        frame (after the resize, before the copy back or the encode) gets its list written on it as the reference's draw_labels writes
        a video frame's (keypoints/text.py: loc="tl", alpha=0.6, font_scale=0.5), all frames of a batch in ONE hh_text_labels_u8_batch
        launch."""
        chunk, options = b.staged.chunk, dict(self.render)
        if options.get("labels") is not None:
            options["labels"] = [self.render["labels"][i] for i in chunk]
        self.model._render_chunk([self.results[i] for i in chunk], b.raw, b.staged.layout.pixel_at, **options)
