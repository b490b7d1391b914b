"""Evaluation of `ClassificationHRNet` on a labelled image set (the reference's `src/classification/bin/eval.py` is a one-line stub and
its README lists this stage as TODO): the scoring tail on the device.

`hh_cls_score_batch` (include/hhrnet.h, where the rule is written) turns a batch of logits into each row's top-k indices and
probabilities, the target's rank and the row's loss, and adds the batch to an accumulator that lives on the device for the whole
evaluation: rows, top-1 / top-k hits, the loss sum, per-class counts and hits and, on request, the confusion matrix.  `ClsEvaluator`
owns that accumulator, `evaluate_images` drives it from raw images (arrays, `JpegImage`s, JPEG bytes) through
`InferenceClassificationModel.prepare_inputs` and the engine: nothing is read back until `result()`.  There is no CPU path.

Tie rule (the project's): equal logits go to the lower index; `torch.topk`, which the reference's metrics use, leaves it unspecified.
"""
from __future__ import annotations

import os
from dataclasses import dataclass

import numpy as np
import torch
from torch import Tensor

from .. import _lib

IMG_EXTENSIONS = (".jpg", ".jpeg", ".png", ".ppm", ".bmp", ".pgm", ".tif", ".tiff", ".webp")  # torchvision.datasets.folder


# the accumulator's 64-byte header, as include/hhrnet.h states it by offset (hh_cls_eval_acc of csrc/cls_score_math.h)
ACC_HEADER = np.dtype({"names": ["rows", "top1", "topk", "bad_target", "nonfinite", "loss_sum", "flags", "N", "with_confusion", "reserved"],
                       "formats": ["<i8"] * 5 + ["<f8", "<u4", "<i4", "<i4", "<i4"], "offsets": [0, 8, 16, 24, 32, 40, 48, 52, 56, 60], "itemsize": 64})


def _header_dtype() -> np.dtype:
    return ACC_HEADER


def state_bytes(num_classes: int, confusion: bool) -> int:
    """The bytes of an accumulator that carry the evaluation: the header, per_class and conf (the call scratch behind them is zero
    between calls)."""
    return _header_dtype().itemsize + 4 * 3 * num_classes + (4 * num_classes * num_classes if confusion else 0)


def parse_state(raw: np.ndarray, num_classes: int, confusion: bool) -> dict:
    """The state bytes of an accumulator -> {"header": 0-d structured array (hh_cls_eval_acc), "per_class": int32 [3,N] (count, top-1
    hits, top-k hits by target class), "conf": int32 [N,N] or None}, as copies."""
    raw = np.ascontiguousarray(raw).view(np.uint8).reshape(-1)
    hb, N = _header_dtype().itemsize, num_classes
    out = {"header": raw[:hb].view(_header_dtype())[0].copy(),
           "per_class": raw[hb:hb + 12 * N].view("<i4").reshape(3, N).copy(), "conf": None}
    if confusion:
        out["conf"] = raw[hb + 12 * N:hb + 12 * N + 4 * N * N].view("<i4").reshape(N, N).copy()
    return out


def merge_states(a: dict, b: dict) -> dict:
    """The sum of two parsed states: integer fields and tables added, loss_sum = a's + b's, flags or-ed (a new dict)."""
    if a["per_class"].shape != b["per_class"].shape or (a["conf"] is None) != (b["conf"] is None) or a["header"]["N"] != b["header"]["N"]:
        raise ValueError("classifier evaluation: the states differ in num_classes or in confusion")
    h = np.zeros((), a["header"].dtype)
    h[...] = a["header"]  # (a copy: np.array() of a structured scalar shares its memory)
    for f in ("rows", "top1", "topk", "bad_target", "nonfinite", "loss_sum"):
        h[f] = a["header"][f] + b["header"][f]
    h["flags"] = a["header"]["flags"] | b["header"]["flags"]
    return {"header": h[()].copy(), "per_class": a["per_class"] + b["per_class"], "conf": None if a["conf"] is None else a["conf"] + b["conf"]}


def pack_state(state: dict) -> np.ndarray:
    """parse_state's inverse: the state bytes (uint8)."""
    parts = [np.frombuffer(np.array(state["header"]).tobytes(), np.uint8), np.ascontiguousarray(state["per_class"], "<i4").view(np.uint8).reshape(-1)]
    if state["conf"] is not None:
        parts.append(np.ascontiguousarray(state["conf"], "<i4").view(np.uint8).reshape(-1))
    return np.concatenate(parts)


def score_logits(logits: Tensor, targets: Tensor | None = None, k: int = 5, acc: Tensor | None = None) -> dict:
    """One hh_cls_score_batch call per HH_CLS_MAX_B rows (one call for any batch an engine forward makes) on the current stream ->
    {"topk_idx": int32 [B,k], "topk_prob": fp32 [B,k], "rank": int32 [B], "row_loss": fp32 [B]} on the device.  `acc`: an accumulator
    set up by hh_cls_eval_reset (ClsEvaluator's), written only when targets are given.  Nothing here waits for the device."""
    if not logits.is_cuda:
        raise _lib.HHError("logits must be a CUDA/HIP tensor: there is no CPU path")
    lib = _lib.load()
    z = logits.detach().to(torch.float32).contiguous()
    if z.dim() != 2:
        raise ValueError(f"score_logits: logits must be [B, N], got {tuple(z.shape)}")
    B, N = z.shape
    t = None
    if targets is not None:
        t = targets.detach().to(z.device, torch.int64).contiguous()
        if t.shape != (B,):
            raise ValueError(f"score_logits: logits {tuple(z.shape)}, targets {tuple(t.shape)}")
    out = {"topk_idx": torch.empty(B, k, device=z.device, dtype=torch.int32), "topk_prob": torch.empty(B, k, device=z.device, dtype=torch.float32),
           "rank": torch.empty(B, device=z.device, dtype=torch.int32), "row_loss": torch.empty(B, device=z.device, dtype=torch.float32)}
    step = _lib.const("CLS_MAX_B")
    for b0 in range(0, B, step):
        n = min(step, B - b0)
        _lib.launch(z.device, lib.hh_cls_score_batch, z[b0:].data_ptr(), None if t is None else t[b0:].data_ptr(), n, N, k, _lib.ptr(acc),
                    out["topk_idx"][b0:].data_ptr(), out["topk_prob"][b0:].data_ptr(), out["rank"][b0:].data_ptr(),
                    out["row_loss"][b0:].data_ptr())
    return out


class ClsEvaluator:
    """The state of one evaluation on the device.  `update(logits, targets)` scores a batch and adds it; `result()` is the one device ->
    host copy.  The accumulator's bytes do not depend on how the rows were split into updates (include/hhrnet.h, ORDER OF loss_sum)."""

    def __init__(self, num_classes: int, k: int = 5, confusion: bool = False, device="cuda:0"):
        lib = _lib.load()
        if not 1 <= k <= _lib.const("CLS_TOPK_MAX"):
            raise ValueError(f"ClsEvaluator: k must lie in 1..{_lib.const('CLS_TOPK_MAX')}")
        self.num_classes, self.k, self.confusion, self.device = int(num_classes), int(k), bool(confusion), torch.device(device)
        nbytes = lib.hh_cls_eval_bytes(self.num_classes, int(self.confusion))
        if nbytes < 0:
            raise _lib.HHError(lib.hh_last_error().decode())
        self._acc = torch.empty(nbytes // 8, device=self.device, dtype=torch.int64)  # (8-byte aligned; a multiple of 8 bytes)
        self.reset()

    def reset(self) -> None:
        _lib.launch(self.device, _lib.load().hh_cls_eval_reset, self._acc.data_ptr(), self.num_classes, int(self.confusion))

    def update(self, logits: Tensor, targets: Tensor) -> dict:
        """Scores logits [B,N] against targets [B] on the current stream and adds the batch to the accumulator -> the per-row outputs
        of `score_logits`, on the device.  Nothing is synchronised."""
        if logits.shape[-1] != self.num_classes:
            raise ValueError(f"ClsEvaluator.update: {logits.shape[-1]} logits per row, evaluator built for {self.num_classes}")
        return score_logits(logits, targets, self.k, self._acc)

    # ------------------------------------------------------------------ reading
    def _state_words(self) -> int:
        return (state_bytes(self.num_classes, self.confusion) + 7) // 8

    def raw_state(self) -> np.ndarray:
        """One device -> host copy of the accumulator's state bytes (uint8)."""
        return self._acc[:self._state_words()].cpu().numpy().view(np.uint8)[:state_bytes(self.num_classes, self.confusion)]

    def state(self) -> dict:
        """{"header", "per_class", "conf"} on the host (`parse_state`): what `merge_` of another evaluator takes."""
        return parse_state(self.raw_state(), self.num_classes, self.confusion)

    def merge_(self, other_state: dict) -> "ClsEvaluator":
        """Adds another accumulator's state (a shard's) to this one: integer fields and tables summed, loss_sum added, flags or-ed."""
        raw = pack_state(merge_states(self.state(), other_state))
        raw = np.concatenate([raw, np.zeros(8 * self._state_words() - raw.size, np.uint8)])
        self._acc[:self._state_words()].copy_(torch.from_numpy(raw.view(np.int64)))
        return self

    def all_reduce(self, group=None) -> "ClsEvaluator":
        """Sharded evaluation: every rank ends with the sum of all ranks' states, merged in rank order (so every rank holds the same
        bytes).  Without an initialised process group this is a no-op."""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
            return self
        states = [None] * dist.get_world_size(group)
        dist.all_gather_object(states, self.state(), group=group)
        self.reset()
        for s in states:
            self.merge_(s)
        return self

    def result(self, allow_bad_targets: bool = False) -> dict:
        """One device -> host copy -> {"n", "top-1_error", f"top-{k}_error" (the key names of the reference's get_metrics), "loss",
        "per_class_count", "per_class_accuracy", f"per_class_top-{k}_accuracy" (NaN where the count is 0), "confusion" (int32 [N,N],
        rows = targets, or None), "bad_target", "nonfinite", "flags"}.  Rows with a target outside [0, num_classes) were not scored;
        unless allow_bad_targets is set their presence raises IndexError, as the training loss does."""
        return summarize(self.state(), self.k, allow_bad_targets)

    def most_confused(self, n: int = 10) -> list:
        """The off-diagonal (target, predicted, count) triples with count > 0, by descending count, then ascending (target, predicted)."""
        if not self.confusion:
            raise ValueError("ClsEvaluator.most_confused: built with confusion=False")
        return most_confused(self.state()["conf"], n)


def summarize(state: dict, k: int, allow_bad_targets: bool = False) -> dict:
    h, pc = state["header"], state["per_class"]
    bad, flags = int(h["bad_target"]), int(h["flags"])
    if flags & _lib.const("CLS_LAYOUT"):
        raise _lib.HHError("classifier evaluation: an update's num_classes did not match the accumulator's")
    if bad and not allow_bad_targets:
        raise IndexError(f"classifier evaluation: {bad} target(s) outside [0, num_classes) (bad_target)")
    n = int(h["rows"])
    nan = float("nan")
    with np.errstate(divide="ignore", invalid="ignore"):
        acc1 = np.where(pc[0] > 0, pc[1] / pc[0].astype(np.float64), np.nan)
        acck = np.where(pc[0] > 0, pc[2] / pc[0].astype(np.float64), np.nan)
    return {"n": n, "top-1_error": 1.0 - int(h["top1"]) / n if n else nan, f"top-{k}_error": 1.0 - int(h["topk"]) / n if n else nan,
            "loss": float(h["loss_sum"]) / n if n else nan, "per_class_count": pc[0].copy(), "per_class_accuracy": acc1,
            f"per_class_top-{k}_accuracy": acck, "confusion": state["conf"], "bad_target": bad, "nonfinite": int(h["nonfinite"]), "flags": flags}


def most_confused(conf: np.ndarray, n: int = 10) -> list:
    c = np.array(conf, dtype=np.int64)
    np.fill_diagonal(c, 0)
    t, p = np.nonzero(c)  # row-major: ascending (target, predicted)
    order = np.argsort(-c[t, p], kind="stable")[:n]
    return [(int(t[i]), int(p[i]), int(c[t[i], p[i]])) for i in order]


@dataclass
class ClsTopK:
    """One image's light record: the k best class indices (the project's order), their probabilities and labels, and with a target its
    label and rank (-1 without one or when it is outside [0, num_classes)).  A non-finite row of logits has indices -1."""
    topk_idx: np.ndarray
    topk_prob: np.ndarray
    labels: list
    rank: int = -1
    target_label: int | str | None = None


def _light_records(chunks: list, idx2label: dict | None, target_labels) -> list:
    """chunks: the per-row outputs of the updates, still on the device -> one host copy each of [B,k] indices, [B,k] probabilities and
    [B] ranks: 2k + 1 numbers per image."""
    idx = torch.cat([c["topk_idx"] for c in chunks]).cpu().numpy()
    prob = torch.cat([c["topk_prob"] for c in chunks]).cpu().numpy()
    rank = torch.cat([c["rank"] for c in chunks]).cpu().numpy()
    label = (lambda j: None if j < 0 else idx2label[j]) if idx2label is not None else (lambda j: None if j < 0 else j)
    return [ClsTopK(idx[i], prob[i], [label(int(j)) for j in idx[i]], int(rank[i]), None if target_labels is None else target_labels[i])
            for i in range(len(idx))]


def infer_topk(model, raw_images: list, target_labels: list | None = None, k: int = 5, max_batch: int = 32) -> list:
    """The light records of `raw_images` without an evaluator (InferenceClassificationModel.infer_topk).  A target label may be a
    class index or a label of the model's idx2label; one that is neither leaves the record's rank at -1."""
    if target_labels is not None and len(target_labels) != len(raw_images):
        raise ValueError("infer_topk: one target label per image")
    t_all = None
    if target_labels is not None:
        label2idx = {v: j for j, v in (model.idx2label or {}).items()}
        as_idx = [int(t) if isinstance(t, (int, np.integer)) else label2idx.get(t, -1) for t in target_labels]
        t_all = torch.as_tensor(np.asarray(as_idx, dtype=np.int64)).to(model.device)
    chunks = []
    for i in range(0, len(raw_images), max_batch):
        with torch.no_grad():
            logits = model.net(model.prepare_inputs(raw_images[i:i + max_batch]))
        chunks.append(score_logits(logits, None if t_all is None else t_all[i:i + max_batch], k))
    return _light_records(chunks, model.idx2label, target_labels) if chunks else []


def evaluate_images(model, images: list, targets, max_batch: int = 32, k: int = 5, confusion: bool = False, records: bool = False,
                    allow_bad_targets: bool = False):
    """Evaluates `model` (an InferenceClassificationModel) on `images` (uint8 arrays, `JpegImage`s or JPEG bytes, mixed: what
    `prepare_inputs` takes) against integer `targets`.  Per chunk of `max_batch`: prepare_inputs, the engine forward, one
    ClsEvaluator.update; nothing is read back until the end.  -> ClsEvaluator.result(), or (result, [ClsTopK]) with records=True."""
    if len(targets) != len(images):
        raise ValueError("evaluate_images: one target per image")
    t_all = torch.as_tensor(np.asarray(targets, dtype=np.int64)).to(model.device)
    ev, chunks = None, []
    for i in range(0, len(images), max_batch):
        with torch.no_grad():
            logits = model.net(model.prepare_inputs(images[i:i + max_batch]))
        if ev is None:
            ev = ClsEvaluator(logits.shape[1], k, confusion, model.device)
        out = ev.update(logits, t_all[i:i + max_batch])
        if records:
            chunks.append(out)
    if ev is None:
        raise ValueError("evaluate_images: no images")
    result = ev.result(allow_bad_targets)
    if not records:
        return result
    labels = [model.idx2label.get(int(t)) if model.idx2label is not None else int(t) for t in np.asarray(targets)]
    return result, _light_records(chunks, model.idx2label, labels)


def image_folder_items(root: str, wordnet_labels: dict | None = None):
    """-> (paths, targets, idx2label) of an ImageNet-style tree root/<class dir>/<image>.  The class index is the position of the
    directory in sorted order (torchvision's ImageFolder rule, which the reference's ImageNet dataset inherits); the images of a class
    come in sorted walk order, files with an image extension only.  wordnet_labels: the reference's {idx: [wordnet id, label]} table
    (its parse_wordnet_labels): idx2label[int(idx)] = label; without it idx2label maps the index to the directory name."""
    classes = sorted(e.name for e in os.scandir(root) if e.is_dir())
    if not classes:
        raise FileNotFoundError(f"image_folder_items: no class directories in {root}")
    paths, targets = [], []
    for idx, name in enumerate(classes):
        for dirpath, _, files in sorted(os.walk(os.path.join(root, name), followlinks=True)):
            for f in sorted(files):
                if f.lower().endswith(IMG_EXTENSIONS):
                    paths.append(os.path.join(dirpath, f))
                    targets.append(idx)
    if wordnet_labels is not None:
        idx2label = {int(idx): labels[1] for idx, labels in wordnet_labels.items()}
    else:
        idx2label = dict(enumerate(classes))
    return paths, targets, idx2label
