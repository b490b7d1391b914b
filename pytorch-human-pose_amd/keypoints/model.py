"""Inference wrapper with the reference's interface.

Stands in for `/root/reference/src/keypoints/model.py:43-111` (`InferenceKeypointsModel`) and
`/root/reference/src/base/model.py:155-175` (checkpoint loading: weights under
ckpt["module"]["model"] or a bare state dict, prefixes `module.` / `_orig_mod.` / `net.` stripped).
"""
from __future__ import annotations

import contextlib

import numpy as np
import torch
from torch import Tensor, nn

from .. import _lib
from .._stage import frames_to_host
from ..optim import clip_grad_norm_
from . import _infer_pipeline as ip
from . import jpeg as jp
from . import pose_score as ps
from ._infer_pipeline import _IMAGE_DESC, plan_multi_scale  # noqa: F401  (read from here by tests and tools)
from .grouping import MPPEHeatmapParser
from .results import InferenceKeypointsResult, transform_coords
from .transforms_utils import COCO_FLIP_INDEX, IMAGENET_MEAN, IMAGENET_STD, dst_to_src_matrix, get_multi_scale_size

COCO_LIMBS = [(15, 13), (13, 11), (16, 14), (14, 12), (11, 12), (5, 11), (6, 12), (5, 6), (5, 7), (6, 8), (7, 9), (8, 10),
              (1, 2), (0, 1), (0, 2), (1, 3), (2, 4), (3, 5), (4, 6)]


def parse_checkpoint(ckpt: dict) -> dict:
    """utils/model.py:166-173"""
    out = {}
    for k, v in ckpt.items():
        for p in ("module.", "_orig_mod.", "net."):
            k = k.replace(p, "")
        out[k] = v
    return out


def checkpoint_weights(ckpt: dict, use_ema: bool = False) -> dict:
    """The state dict of the net inside a loaded checkpoint: ckpt["module"]["model"], or the checkpoint itself where it is a bare state
    dict; with use_ema the averaged weights under ckpt["module"]["ema"]["model"] (KeyError naming the missing entry otherwise)."""
    if use_ema:
        node, path = ckpt, "checkpoint"
        for key in ("module", "ema", "model"):
            if not isinstance(node, dict) or key not in node:
                raise KeyError(f'load_checkpoint(use_ema=True): the checkpoint has no ["module"]["ema"]["model"] entry ({path} lacks "{key}")')
            node, path = node[key], f'{path}["{key}"]'
        return node
    return ckpt["module"]["model"] if "module" in ckpt.keys() else ckpt


class BaseModel:
    """What the trainer-facing model wrappers share (base/model.py:15-131 without the export / summary helpers: onnx, torchinfo are
    out of scope): KeypointsModel below and classification/model.py's ClassificationModel."""

    EXAMPLE_SIZE = 512

    def __init__(self, net: nn.Module, input_names: list, output_names: list):
        self.net = net
        self.input_names, self.output_names = input_names, output_names

    def _bare(self) -> nn.Module:
        from torch.nn.parallel import DistributedDataParallel as DDP
        return self.net.module if isinstance(self.net, DDP) else self.net

    def forward(self, images: Tensor):
        return self.net(images)

    def init_pretrained_weights(self, ckpt: dict) -> None:
        """base/model.py:101-123: load the checkpoint entries whose names exist here, ignore the rest."""
        net = self._bare()
        names = {n for n, _ in net.named_parameters()} | {n for n, _ in net.named_buffers()}
        net.load_state_dict({k: v for k, v in parse_checkpoint(ckpt).items() if k in names}, strict=False)

    def to_CUDA(self, device_id: int) -> None:
        self.net = self.net.cuda(device_id)

    def to_DDP(self, device_id: int, use_batchnorm: bool, bf16_gradients: bool = False) -> None:
        """base/model.py:36-48.  `use_batchnorm` is the reference's SyncBatchNorm switch (its trainer's default; the HigherHRNet
        experiment file sets `sync_batchnorm: false`): here the
        BatchNorm leaves stay what they are and the training forward shares their statistics across the ranks of the default
        process group (hh_bn_train_stats -> all-reduce -> hh_bn_train_normalize).  Gradients: torch DDP's bucketed
        all-reduce on RCCL, overlapped with the backward; `bf16_gradients=True` sends the buckets as bf16."""
        from torch.nn.parallel import DistributedDataParallel as DDP
        self.net.sync_batchnorm = True if use_batchnorm else None
        self.net = DDP(self.net, device_ids=[device_id])
        if bf16_gradients:  # not in the reference: halves the 114.6 MB (W32) the ring moves per step; the optimizer still sees fp32
            from torch.distributed.algorithms.ddp_comm_hooks import default_hooks
            self.net.register_comm_hook(None, default_hooks.bf16_compress_hook)

    @property
    def device(self):
        return next(self._bare().parameters()).device

    def freeze(self) -> None:
        for p in self.net.parameters():
            p.requires_grad = False

    def state_dict(self) -> dict:
        return self._bare().state_dict()

    def load_state_dict(self, state_dict: dict) -> None:
        self._bare().load_state_dict(state_dict)

    def example_input(self) -> dict[str, Tensor]:
        return {"images": torch.randn(1, 3, self.EXAMPLE_SIZE, self.EXAMPLE_SIZE, device=self.device)}


class KeypointsModel(BaseModel):
    """Training-side model wrapper: `KeypointsModel` (keypoints/model.py:15-40) on `BaseModel` (base/model.py:15-131)
    without the export / summary helpers (onnx, torchinfo: out of scope)."""

    def __init__(self, net: nn.Module):
        super().__init__(net, ["images"], ["keypoints"])

    def init_weights(self) -> None:
        """keypoints/model.py:19-34: conv / transposed-conv weights ~ N(0, 0.001), their biases 0, BatchNorm weight 1 / bias 0."""
        net = self._bare()
        for m in net.modules():
            if isinstance(m, (nn.Conv2d, nn.ConvTranspose2d)):
                nn.init.normal_(m.weight, std=0.001)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)
        net.mark_dirty()


class KeypointsModule:
    """`KeypointsModule.training_step` (keypoints/module.py:43-71): forward, AE loss, backward, optimizer step.  The reference
    runs under fp16 autocast with one GradScaler per optimizer, whose state goes into every checkpoint (base/module.py:71,109-127).
    precision="fp16" is that: fp16 activations (HigherHRNet.set_train_precision), `scalers = {"optim": GradScaler}`, and the
    reference's sequence scale(loss).backward() / scaler.step(optimizer) / scaler.update(); the metrics are the unscaled values.
    precision="bf16" (default) keeps activations in bf16, which needs no scaler: `scalers` is {}.  Parameters are fp32 either way.
    eval_dtype: the element type of the inference engine that `validation_step` runs ("bf16" / "fp16" / ..., the net's DTYPES).  None
    (default) leaves the net's engine as it is; a name calls `net.set_engine_dtype` once, here -- eval_dtype="fp16" makes the
    validation of an fp16 training run infer in the precision it trains in (and the reference validates in).
    max_grad_norm (not in the reference; None = off, the step is exactly the sequence above): the gradients are clipped to this global
    norm (grad_norm_type: 2 or inf) between the backward and the step -- bf16: backward, clip, step; fp16: scale(loss).backward(),
    scaler.unscale_, clip, scaler.step, scaler.update -- and metrics["grad_norm"] is the norm before clipping.  optim.clip_grad_norm_
    does it: on the optimizer's device table for an optimizer of ..optim, with torch's function for any other.
    ema_decay (not in the reference; None = off: the step as before, bit for bit, and no "ema" entry in state_dict()): a number keeps
    an exponential moving average of the weights, `self.ema = optim.ModelEMA(net, optimizer, ema_decay, ema_warmup, ema_use_buffers)`.
    With an optimizer of ..optim it is updated inside the step launch and follows the scaler's skip; after any other optimizer's step
    training_step calls ema.update() (an fp16 step skipped by torch's scaler is then still averaged and counted, as by torch's
    AveragedModel: the host cannot know).  validation_step runs on the averaged weights (ema.applied()) and state_dict() carries them."""

    PRECISIONS = ("bf16", "fp16")

    def __init__(self, model: KeypointsModel, loss_fn, optimizer: torch.optim.Optimizer, precision: str = "bf16", eval_dtype: str | None = None,
                 max_grad_norm: float | None = None, grad_norm_type: float = 2.0, ema_decay: float | None = None, ema_warmup: bool = False,
                 ema_use_buffers: bool = False):
        if precision not in self.PRECISIONS:
            raise ValueError(f"KeypointsModule: precision {precision!r} is not one of {self.PRECISIONS}")
        self.model, self.loss_fn, self.optimizer, self.precision = model, loss_fn, optimizer, precision
        self.max_grad_norm, self.grad_norm_type = max_grad_norm, grad_norm_type
        # (an optimizer of ..optim gets the scaler whose non-finite check is one launch over its table; any other, torch's own)
        from ..optim import GradScaler, ModelEMA, is_device_optimizer
        self.ema = None if ema_decay is None else ModelEMA(model.net, optimizer, ema_decay, ema_warmup, ema_use_buffers)
        scaler_cls = GradScaler if is_device_optimizer(optimizer) else torch.amp.GradScaler
        self.scalers: dict = {"optim": scaler_cls("cuda")} if precision == "fp16" else {}
        if max_grad_norm is not None and is_device_optimizer(optimizer):
            optimizer.collect_grad_stats = True  # the scaler's unscale launch leaves the statistics the clip needs
        model._bare().set_train_precision(precision)
        self.eval_dtype = eval_dtype
        if eval_dtype is not None:
            model._bare().set_engine_dtype(eval_dtype)

    def state_dict(self) -> dict:
        """The module's own checkpoint entries in the reference's format (base/module.py:109-127): {"scalers": {name: state}}, and
        with ema_decay set {"ema": ModelEMA.state_dict()} next to it."""
        sd = {"scalers": {name: scaler.state_dict() for name, scaler in self.scalers.items()}}
        if self.ema is not None:
            sd["ema"] = self.ema.state_dict()
        return sd

    def load_state_dict(self, state_dict: dict) -> None:
        for name, scaler in self.scalers.items():
            scaler.load_state_dict(state_dict["scalers"][name])
        if self.ema is not None:
            self.ema.load_state_dict(state_dict["ema"])

    def batch_to_device(self, batch):
        images, heatmaps, masks, joints = batch
        dev = self.model.device
        return images.to(dev), [h.to(dev, non_blocking=True) for h in heatmaps], [m.to(dev, non_blocking=True) for m in masks], joints

    def training_step(self, batch, batch_idx: int = 0) -> dict[str, float]:
        images, heatmaps, masks, joints = batch
        stages_hms, tags = self.model.net(images)
        hm_losses, push_losses, pull_losses = self.loss_fn.calculate_loss(stages_hms, tags, heatmaps, masks, joints)
        loss = 0
        for hl in hm_losses:
            loss = loss + hl
        loss = loss + push_losses[0] + pull_losses[0]
        self.optimizer.zero_grad()
        scaler = self.scalers.get("optim")
        grad_norm = None
        if scaler is None:
            loss.backward()
            if self.max_grad_norm is not None:
                grad_norm = clip_grad_norm_(self.optimizer, self.max_grad_norm, self.grad_norm_type)
            self.optimizer.step()
        else:  # (module.py:55-60; a step whose gradients hold an inf / NaN is skipped and the scale halved)
            scaler.scale(loss).backward()
            if self.max_grad_norm is not None:
                scaler.unscale_(self.optimizer)
                grad_norm = clip_grad_norm_(self.optimizer, self.max_grad_norm, self.grad_norm_type)
            scaler.step(self.optimizer)
            scaler.update()
        if self.ema is not None and self.ema.optimizer is None:  # (attached to a device optimizer it was updated inside the step)
            self.ema.update()
        self.model._bare().mark_dirty()
        metrics = {"loss": loss.detach().item()}
        if grad_norm is not None:
            metrics["grad_norm"] = grad_norm.item()
        for i, hl in enumerate(hm_losses):
            metrics[f"hm_{i}_loss"] = hl.item()
        for i in range(len(push_losses)):
            metrics[f"push_{i}_loss"] = push_losses[i].item()
            metrics[f"pull_{i}_loss"] = pull_losses[i].item()
        return metrics

    def validation_step(self, batch, batch_idx: int = 0):
        """`KeypointsModule.validation_step` (keypoints/module.py:73-111): forward, the same losses as the training step (no
        backward), and one KeypointsResult per image decoded at the validation thresholds (20 people, det 0.1, tag 1.0).  The
        reference decodes image by image on the host; here the whole batch goes through one hh_decode."""
        from .results import KeypointsResult
        images, heatmaps, masks, joints = batch
        with torch.no_grad(), (self.ema.applied() if self.ema is not None else contextlib.nullcontext()):
            stages_hms, tags = self.model.net(images)
            hm_losses, push_losses, pull_losses = self.loss_fn.calculate_loss(stages_hms, tags, heatmaps, masks, joints)
        loss = hm_losses[0] + hm_losses[1] + push_losses[0] + pull_losses[0]
        metrics = {"loss": loss.detach().item()}
        for i, hl in enumerate(hm_losses):
            metrics[f"hm_{i}_loss"] = hl.item()
        for i in range(len(push_losses)):
            metrics[f"push_{i}_loss"] = push_losses[i].item()
            metrics[f"pull_{i}_loss"] = pull_losses[i].item()
        stages_hms, tags = [h.detach().float() for h in stages_hms], tags.detach().float()
        # one parser (= one device workspace) for the life of the module, not one per step
        K = stages_hms[0].shape[1]
        parser = getattr(self, "_val_parser", None)
        if parser is None or parser.num_kpts != K:
            parser = self._val_parser = MPPEHeatmapParser(K, 20, 0.1, 1.0)
        cpu_images = images.detach().cpu()
        results = [KeypointsResult(cpu_images[i], [h[i:i + 1] for h in stages_hms], tags[i:i + 1], COCO_LIMBS, 20, 0.1, 1.0, parser=parser)
                   for i in range(len(cpu_images))]
        KeypointsResult.set_preds_batch(results, stages_hms, tags)
        return metrics, results


# one source of hh_multi_scale_aggregate
_ScaleSrc = _lib.struct_ctype("hh_scale_src")


class InferenceKeypointsModel:
    limbs = COCO_LIMBS

    def __init__(self, net: nn.Module, det_thr: float = 0.05, tag_thr: float = 0.5, use_flip: bool = False,
                 input_size: int = 512, max_num_people: int = 30, device: str = "cuda:0", ckpt_path: str | None = None):
        self.net = net.to(device)
        self.net.eval()
        self.device = device
        self.input_size = input_size
        self.det_thr, self.tag_thr = det_thr, tag_thr
        self.max_num_people = max_num_people
        self.use_flip = use_flip
        self._lib = _lib.load()
        self._parser = MPPEHeatmapParser(net.num_kpts, max_num_people, det_thr, tag_thr)
        self._perm = np.asarray(COCO_FLIP_INDEX, np.int32)
        self._stream = None       # highest-priority compute stream (created on first use: needs the device)
        self._copy_stream = None  # infer_images: host -> device of the next batch's pixels
        self._d2h_stream = None   # infer_images: result copies, beside the next batch's launches
        self._out_ring: dict = {}  # infer_images: pinned result buffers per pipeline slot and shape
        self._score_stage = None  # infer_images(score=...): pinned buffers of the target tables, one per pipeline slot
        if ckpt_path is not None:
            self.load_checkpoint(ckpt_path)

    def load_checkpoint(self, ckpt_path: str, use_ema: bool = False) -> None:
        """base/model.py:167-175: a trainer checkpoint keeps the weights under ["module"]["model"]; a bare state dict (the
        published pretrained/higher_hrnet_32.pt) is loaded as it is.  use_ema=True loads the averaged weights a module trained with
        ema_decay has put under ["module"]["ema"]["model"] instead, and raises KeyError where there are none."""
        ckpt = torch.load(ckpt_path, map_location="cpu")
        self.net.load_state_dict(parse_checkpoint(checkpoint_weights(ckpt, use_ema)))

    def prepare_input_scaled(self, image: np.ndarray, current_scale: float, min_scale: float):
        """prepare_input for one entry of a multi-scale test (get_multi_scale_size, base/transforms/utils.py:60-86)."""
        size, center, scale = get_multi_scale_size(image, self.input_size, current_scale, min_scale)
        m = dst_to_src_matrix(center, scale, size)  # destination -> source, as cv2.warpAffine inverts the forward matrix
        if hasattr(image, "stage"):  # a jpeg.JpegImage: only its bytes cross, its pixels are formed on the device (a bad stream raises)
            raw = jp.decode_jpeg_device([image], device=self.device)[0]
        else:
            raw = torch.from_numpy(np.ascontiguousarray(image, dtype=np.uint8)).to(self.device)
        x = torch.empty((1, 3, size[1], size[0]), device=self.device, dtype=torch.float32)
        _lib.launch(x.device, self._lib.hh_preprocess_u8, raw.data_ptr(), image.shape[0], image.shape[1], m.ctypes.data, x.data_ptr(),
                    size[1], size[0], IMAGENET_MEAN.ctypes.data, IMAGENET_STD.ctypes.data)
        self._keep_raw = raw
        return x, center, scale

    @torch.no_grad()
    def multi_scale_maps(self, raw_image: np.ndarray, scales=(0.5, 1.0, 2.0)):
        """Multi-scale (+ flip if use_flip) test of BASELINE.json configs[3] -- an EXTENSION, the reference has no
        aggregation code.  Every scale runs the same forward/flip-merge as a single-scale call; its two stage heatmaps
        are bilinearly resized to the scale-1 pass's 1/4 and 1/2 resolutions and averaged over the scales
        (hh_resize_accumulate); tags are taken from the scale-1 pass only (as the HigherHRNet paper's test code does
        for the grouping keys).  Returns ([hm_1/4, hm_1/2], tags_list, x_base, center, scale) ready for from_preds."""
        assert 1.0 in scales, "the scale-1 pass provides the tags and the output geometry"
        mn = min(scales)
        xb, center, scale = self.prepare_input_scaled(raw_image, 1.0, mn)
        hms_b, tags_b = self.forward_tta(xb)
        K = self.net.num_kpts
        acc = [torch.empty_like(hms_b[0].contiguous()), torch.empty_like(hms_b[1].contiguous())]
        wgt = 1.0 / len(scales)
        first = True
        for s in scales:
            hms = hms_b if s == 1.0 else self.forward_tta(self.prepare_input_scaled(raw_image, s, mn)[0])[0]
            for st in range(2):
                src = hms[st]
                _lib.launch(xb.device, self._lib.hh_resize_accumulate, src.data_ptr(), src.stride(0), 1, K, src.shape[2], src.shape[3],
                            acc[st].data_ptr(), acc[st].stride(0), acc[st].shape[2], acc[st].shape[3], wgt, int(first))
            first = False
        return acc, [t.contiguous() for t in tags_b], xb, center, scale

    def call_multi_scale(self, raw_image: np.ndarray, annot: list | None = None, scales=(0.5, 1.0, 2.0)) -> InferenceKeypointsResult:
        hms, tags, xb, center, scale = self.multi_scale_maps(raw_image, scales)
        self.model_input_shape = tuple(xb.shape[-2:])
        return InferenceKeypointsResult.from_preds(raw_image, annot, xb[0], hms, tags, self.limbs, scale, center, self.det_thr,
                                                   self.tag_thr, self.max_num_people, parser=self._parser)

    def prepare_input(self, image: np.ndarray):
        """model.py:70-76: resize-align -> ToTensor -> Normalize -> [1,3,h,w] on device.  Only the raw uint8 image
        crosses PCIe; warp + normalisation run in hh_preprocess_u8."""
        return self.prepare_input_scaled(image, 1, 1)

    def _forward_with_mirror(self, x: Tensor) -> tuple[Tensor, Tensor]:
        """forward_raw of the images [:B] and their mirror images [B:] (model.py:85-86), nothing merged yet."""
        B, _, H, W = x.shape
        # the images and their mirror images as ONE batch of 2B: images of a batch are independent (same bits as two passes), and
        # a forward costs ~2 ms of launch structure whatever the batch -- a single image is a chain of ~350 dependent launches
        x2 = torch.empty((2 * B, 3, H, W), device=x.device, dtype=x.dtype)
        x2[:B].copy_(x)
        _lib.launch(x.device, self._lib.hh_flip_images, x.data_ptr(), x2[B:].data_ptr(), B, 3, H, W)
        return self.net.forward_raw(x2)

    @torch.no_grad()
    def _multi_scale_maps_batch(self, scales: tuple, sub_batches: list, x1: Tensor, prepare) -> tuple[list[Tensor], list[Tensor]]:
        """multi_scale_maps for the images of one chunk (plan_multi_scale): `x1` = their scale-1 model inputs [n,3,h,w],
        `prepare(si)` = their inputs at scales[si].  Every scale runs its sub-batches as forwards of their own; the scale-1 pass is
        forward_tta as it stands (its hh_flip_merge stays: the tags come from this pass, and its merged maps enter the aggregation
        as plain sources), the other scales' flipped passes are merged inside hh_multi_scale_aggregate.  One aggregation launch
        per stage and per image range between two sub-batch boundaries of any scale.  -> ([hm_1/4, hm_1/2] averaged, tags)."""
        K = self.net.num_kpts
        n, _, h, w = x1.shape
        i1 = scales.index(1.0)
        parts: list = []  # per scale: (lo, hi, (stage-0 maps, their flipped pass or None), (stage-1 maps, ...)) per sub-batch
        tags = None
        for si in range(len(scales)):
            xs = x1 if si == i1 else prepare(si)
            per = []
            for lo, hi in sub_batches[si]:
                xb = xs[lo:hi]
                if si == i1:
                    assert (lo, hi) == (0, n), "the plan runs the scale-1 pass of a chunk as one forward"
                    hms, tags = self.forward_tta(xb)
                    per.append((lo, hi, (hms[0], None), (hms[1], None)))
                elif not self.use_flip:
                    init, dec = self.net.forward_raw(xb)
                    per.append((lo, hi, (init, None), (dec, None)))
                else:
                    init2, dec2 = self._forward_with_mirror(xb)
                    per.append((lo, hi, (init2[:hi - lo], init2[hi - lo:]), (dec2[:hi - lo], dec2[hi - lo:])))
            parts.append(per)
        acc = [torch.empty((n, K, h // 4, w // 4), device=x1.device, dtype=torch.float32),
               torch.empty((n, K, h // 2, w // 2), device=x1.device, dtype=torch.float32)]
        wgt = 1.0 / len(scales)
        cuts = sorted({lo for per in parts for lo, _, _, _ in per} | {n})
        table = (_ScaleSrc * len(scales))()
        for a, b in zip(cuts[:-1], cuts[1:]):
            for st in range(2):
                for si, per in enumerate(parts):
                    lo, _, *stages = next(p for p in per if p[0] <= a < p[1])
                    hm, hmf = stages[st]  # [*, >=K, h_s, w_s]: the heatmaps are the first K channels
                    table[si] = _ScaleSrc(hm.data_ptr() + 4 * (a - lo) * hm.stride(0), hm.stride(0),
                                          hmf.data_ptr() + 4 * (a - lo) * hmf.stride(0) if hmf is not None else None,
                                          hmf.stride(0) if hmf is not None else 0, hm.shape[2], hm.shape[3], wgt)
                dst = acc[st][a:b]
                _lib.launch(x1.device, self._lib.hh_multi_scale_aggregate, table, len(scales), self._perm.ctypes.data, b - a, K, dst.data_ptr(),
                            dst.stride(0), dst.shape[2], dst.shape[3])
        return acc, tags

    @torch.no_grad()
    def forward_tta(self, x: Tensor) -> tuple[list[Tensor], list[Tensor]]:
        """model.py:79-94 on a batch [B,3,h,w]: net forward (+ flipped pass, un-flip, joint permutation,
        heatmap average). Returns ([hm_1/4, hm_1/2], [tags] or [tags, tags_flipped])."""
        K = self.net.num_kpts
        if not self.use_flip:
            init, dec = self.net.forward_raw(x)
            return [init[:, :K], dec], [init[:, K:]]
        B, _, H, W = x.shape
        init2, dec2 = self._forward_with_mirror(x)
        init, init_f, dec, dec_f = init2[:B], init2[B:], dec2[:B], dec2[B:]
        tags2 = torch.empty((B, K, H // 4, W // 4), device=x.device, dtype=torch.float32)
        hq, wq = H // 4, W // 4
        p = self._perm.ctypes.data
        # stage 0: heatmaps = init[:, :K] (batch stride 2K planes), tags = init[:, K:]
        _lib.launch(x.device, self._lib.hh_flip_merge, init.data_ptr(), init.stride(0), init_f.data_ptr(), init_f.stride(0),
                    init_f[:, K:].data_ptr(), init_f.stride(0), tags2.data_ptr(), tags2.stride(0), p, B, K, hq, wq)
        _lib.launch(x.device, self._lib.hh_flip_merge, dec.data_ptr(), dec.stride(0), dec_f.data_ptr(), dec_f.stride(0), None, 0, None, 0, p,
                    B, K, 2 * hq, 2 * wq)
        return [init[:, :K], dec], [init[:, K:], tags2]

    @torch.no_grad()
    def infer_batch_device(self, x: Tensor):
        """Batched forward + decode entirely on the device -> (joints [B,M,K,3+E], scores [B,M], num_people [B])."""
        hms, tags = self.forward_tta(x)
        return self._parser.decode_batch_device(hms[0], hms[1], tags, adjust=True, refine=True)

    def _on_fast_stream(self, fn):
        """Run `fn` on this model's highest-priority stream, ordered after / before the caller's current stream.  A single
        image is a chain of ~350 small dependent launches; on this stack they follow each other faster on a high-priority
        queue (the engine's branch lanes take the priority of the stream they are forked from)."""
        if self._stream is None:
            self._stream = torch.cuda.Stream(self.device, priority=torch.cuda.Stream.priority_range()[1])
        cur = torch.cuda.current_stream(self.device)
        self._stream.wait_stream(cur)
        with torch.cuda.stream(self._stream):
            out = fn()
        cur.wait_stream(self._stream)
        return out

    def _geometry(self, image: np.ndarray):
        """Resize-align geometry of one raw image: ((w, h) of the model input, center, scale, destination->source 2x3 matrix)."""
        size, center, scale = get_multi_scale_size(image, self.input_size, 1, 1)
        return size, center, scale, dst_to_src_matrix(center, scale, size)

    @torch.no_grad()
    def infer_images(self, raw_images: list[np.ndarray], annots: list | None = None, max_batch: int = 32,
                     scales=None, render: dict | None = None, tracker=None, score: str | None = None) -> list[InferenceKeypointsResult]:
        """The batched path behind the reference's single-image interface (`__call__` per image, bin/eval.py:18-49): every image gets
        the result `self(image, annot)` returns, from batches of up to `max_batch` images of one model-input shape that run as a
        two-deep pipeline.  The stages are in keypoints/_infer_pipeline.py; each option is described where it is implemented:
        `scales` = tuple of scales, the multi-scale test of `call_multi_scale` for every image: `plan_batches`, `Pipeline._launch`.
        `render` = dict(color_mode, alpha, bgr, out_height, jpeg, labels): every result carries `.rendered` (or `.rendered_jpeg`):
        `check_options`, `Pipeline._render`.
        `tracker` = a keypoints.tracking.PoseTracker with one stream, the images being consecutive frames of ONE clip: results gain
        `.track_ids` and `.kpts_coords_smooth`: `plan_batches`, `Pipeline._launch`, `Pipeline.collect`.
        `score` = "oks" or "pckh": every image whose annot is not None is scored against it on the device (keypoints/pose_score.py):
        `check_options`, `Pipeline.stage`, `Pipeline._launch`, `Pipeline._attach_scores`.
        An entry of `raw_images` may also be the `bytes` / `bytearray` / `memoryview` of a JPEG file or a `jpeg.JpegImage`, mixed freely
        with arrays; bytes become `JpegImage(data, index="device")`: no Huffman pass and no pixel array on the host.  A file the decoder
        refuses by name (progressive, CMYK, ...) is refused at `JpegImage(...)`: pass it as a Pillow array; there is no silent
        fallback: `Pipeline.stage`, `Pipeline._launch`, `Pipeline.collect`.
        With an option left at None nothing of the pipeline changes; a batch of arrays takes exactly the path it took before.
        `self.last_h2d_bytes` keeps the bytes the call uploaded."""
        score_vars = ip.check_options(render, tracker, score, len(raw_images), self._parser.num_kpts, self._parser.max_num_people)
        if score is not None and self._score_stage is None:
            self._score_stage = [ps.TableStage(), ps.TableStage()]  # pinned table buffers, one per pipeline slot
        raw_images = [jp.JpegImage(img, index="device") if isinstance(img, (bytes, bytearray, memoryview)) else img for img in raw_images]
        annots = annots if annots is not None else [None] * len(raw_images)
        self.last_h2d_bytes = 0
        plan = ip.plan_batches(raw_images, self.input_size, scales, max_batch, tracker)
        run = ip.Pipeline(self, plan, raw_images, annots, render, tracker, score, score_vars)
        pending = None
        for sizes, chunk, subs in plan.jobs:
            batch = run.enqueue(run.stage(sizes, chunk, subs))
            if pending is not None:
                run.collect(pending)
            pending = batch
        if pending is not None:
            run.collect(pending)
        return run.results

    def _render_chunk(self, results: list, raw: Tensor, offs, color_mode: str = "person", alpha: float = 0.8, bgr: bool = False,
                      out_height: int | None = None, jpeg: dict | None = None, labels: list | None = None) -> None:
        """`.rendered` of the results of one batch: one render launch on the batch's staged pixels (`raw`: the device copy of the
        staging buffer, image j's h * w * 3 bytes from offs[j]), the optional resizes, one pinned buffer back.  With `jpeg`:
        `.rendered_jpeg` instead, one encode call on the device frames, only the compressed bytes back.  With `labels` (one list of
        strings or None per result): one text launch on the finished device frames in front of either."""
        from . import visualization as vz
        cur = torch.cuda.current_stream(self.device)
        raw.record_stream(cur)
        frames, tables = [], []
        for j, r in enumerate(results):
            shape = r.raw_shape  # (of a JPEG input too: its pixels were formed on the device, at offs[j])
            frames.append(raw[int(offs[j]):int(offs[j]) + shape[0] * shape[1] * 3].view(shape))
            by_id = color_mode == "track"
            tables.append(vz.build_primitives(r.kpts_coords_smooth if by_id else r.kpts_coords, r.kpts_scores, r.limbs, r.det_thr, color_mode,
                                              vz.DEFAULT_PALETTE, alpha, ids=r.track_ids if by_id else None))
        out = vz.render_frames_device(frames, tables, alpha, bgr)
        if out_height is not None:
            out = [f if f.shape[0] == out_height else vz.resize_device(f, int(out_height * f.shape[1] / f.shape[0]), out_height) for f in out]
        if labels is not None:
            from . import text as tx
            tx.put_txt_device(out, [tx.video_table(int(f.shape[0]), int(f.shape[1]), lines) if lines is not None else np.zeros(0, tx.PRIM)
                                    for f, lines in zip(out, labels)])
        if jpeg is not None:
            for r, data in zip(results, jp.encode_jpeg_device(out, bgr=bgr, **jpeg)):
                r.rendered_jpeg = data
            return
        for r, frame in zip(results, frames_to_host(out)):
            r.rendered = frame

    def _single(self, raw_image, annot, tracker=None) -> InferenceKeypointsResult:
        """One image on the fast stream: prepare_input, forward_tta, hh_decode, (`tracker`: one hh_track_step behind the decode on the
        same stream, one frame of the tracker's one stream,) the result as `InferenceKeypointsResult.from_preds` builds it."""
        def run():
            x, center, scale = self.prepare_input(raw_image)
            h, w = self.model_input_shape = tuple(x.shape[-2:])
            hms, tags = self.forward_tta(x)
            out = self._parser.decode_batch_device(hms[0], hms[1], tags, adjust=True, refine=True)
            track = tracker.update_device(*out, frames_per_stream=1) if tracker is not None else None
            joints, scores = self._parser.to_lists(*out)[0]
            coords = transform_coords(joints[..., :2], center, scale, (w, h))
            result = InferenceKeypointsResult(raw_image, annot, x[0], coords, joints[..., 2], joints[..., 3:], scores, self.det_thr, self.tag_thr,
                                              self.limbs, hms, tags)
            if track is not None:
                p = len(joints)
                result.track_ids = track[0][0, :p].cpu().numpy()
                result.kpts_coords_smooth = transform_coords(track[1][0, :p].cpu().numpy(), center, scale, (w, h)).astype(coords.dtype)
            return result
        return self._on_fast_stream(run)

    def _call_tracked(self, raw_image: np.ndarray, tracker) -> InferenceKeypointsResult:
        """`self(raw_image, None)` with one hh_track_step behind the decode on the same stream (one frame of the tracker's one stream)."""
        if tracker.streams != 1:
            raise ValueError("video_frame: the tracker must have one stream")
        size = get_multi_scale_size(raw_image, self.input_size, 1, 1)[0]
        tracker.bind_input_shape((size[1], size[0]))  # (raises before any launch)
        return self._single(raw_image, None, tracker)

    def video_frame(self, image: np.ndarray, tracker=None, jpeg: dict | None = None, labels: list | None = None):
        """`video_processing_fn` (keypoints/bin/inference.py:49-75) -> (result, out_frame): one inference,
        the people ordered by their mean tag (same colours for the same person from frame to frame), limb colours at alpha 0.65 with
        thr = det_thr, B,G,R order, resized to height 640 (new_w = int(640 * w / h); no resize launch when h == 640).  The frame is
        drawn from the uint8 pixels prepare_input already put on the device: the raw image crosses PCIe once, the finished frame
        comes back through one pinned buffer.
        `tracker` = a keypoints.tracking.PoseTracker with one stream (an extension): the frame is the next one of the tracker's clip; the
        result carries `.track_ids` and `.kpts_coords_smooth` (see infer_images) and the overlay draws the smoothed coordinates, every
        person in the colour of its id (color_mode "track") instead of the tag order and the limb colours.
        `jpeg` = dict(quality=90, subsampling="420") (an extension): out_frame is the 640-high frame as a JFIF stream (bytes), encoded on the
        GPU (keypoints/jpeg.py) with bgr=True, so that the stream holds the true colours; what `MJPEGWriter.write` takes.  The raw frame
        is not copied back.
        `labels` = a list of strings (`keypoints.text.video_labels(idx, num_frames, model_input_shape, speed_ms)` gives the reference's):
        written on the finished 640-high B,G,R frame as InferenceVideoDataset.draw_labels writes them (base/datasets/video.py:168-176:
        loc="tl", alpha=0.6, font_scale=0.5) by one hh_text_labels_u8_batch launch on the device frame, before it is copied back or
        encoded: with `jpeg` the labelled frame never exists on the host.  labels=None: no text launch, the frame as before."""
        from . import visualization as vz
        if tracker is not None:
            result = self._call_tracked(image, tracker)
            table = vz.build_primitives(result.kpts_coords_smooth, result.kpts_scores, result.limbs, result.det_thr, "track", vz.DEFAULT_PALETTE, 0.65,
                                        ids=result.track_ids)
        else:
            result = self(image, None)
            order = np.argsort(result.kpts_tags.mean(axis=1)[:, 0])
            table = vz.build_primitives(result.kpts_coords[order], result.kpts_scores[order], result.limbs, result.det_thr, "limb", vz.DEFAULT_PALETTE, 0.65)
        raw = self._keep_raw  # uint8 [h,w,3] on the device (prepare_input)
        frame = vz.render_frames_device([raw], [table], 0.65, bgr=True)[0]
        h, w = raw.shape[:2]
        if h != 640:
            frame = vz.resize_device(frame, int(640 * w / h), 640)
        if labels is not None:
            from . import text as tx
            tx.put_txt_device([frame], [tx.video_table(int(frame.shape[0]), int(frame.shape[1]), labels)])
        if jpeg is not None:
            return result, jp.encode_jpeg_device([frame], bgr=True, **jpeg)[0]
        return result, vz.to_host(frame)

    def __call__(self, raw_image: np.ndarray, annot: list | None) -> InferenceKeypointsResult:
        """model.py:78-111.  `raw_image` may also be the bytes of a JPEG file or a jpeg.JpegImage (see infer_images): the bytes cross,
        the index (of bytes: on the device) and the pixels are formed on the GPU, and the result's `.raw_image` is decoded on the host
        on first access."""
        if isinstance(raw_image, (bytes, bytearray, memoryview)):
            raw_image = jp.JpegImage(raw_image, index="device")
        return self._single(raw_image, annot)
