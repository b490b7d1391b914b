"""`ClassificationModule.training_step` / `validation_step` (src/classification/module.py:45-82) on the HIP training kernels.

Precision: the reference trains this net in fp32 without a loss scaler; here the activations of the training forward / backward are
bf16 (a stated deviation: the training kernels are 16-bit; bf16 keeps fp32's exponent range, so no scaler is needed), parameters,
their gradients, the pooled features, the Linear and the loss are fp32.  The metrics come from the loss kernel's result record:
one device -> host read per step (the reference copies the logits to the host and runs topk there)."""
from __future__ import annotations

import contextlib
from dataclasses import dataclass

import numpy as np
import torch
from torch import Tensor

from ..optim import ModelEMA, clip_grad_norm_
from .loss import ClassificationLoss
from .model import ClassificationModel


@dataclass
class ClassificationResult:
    """One validation image (classification/results.py:13-36): its logits, target and prediction (the arg-max, the lower index on a
    tie).  `plot()` needs `model_input_image` (the normalised [3,H,W] input, kept on the device) and `idx2label`; validation_step
    fills both."""
    logits: np.ndarray
    target: int
    prediction: int
    target_label: str | int | None = None
    model_input_image: Tensor | None = None
    idx2label: dict | None = None

    def _plot_device(self) -> dict[str, Tensor]:
        """results.py:26-36: probs = (exp(logits) + eps) / sum, eps of the logits' dtype; plot_top_preds on the un-normalised model
        input (hh_unnormalize_u8), drawn by one text launch.  -> {"top_probs": device uint8 [H,W,3]}."""
        from ..keypoints import visualization as vz
        from .visualization import plot_top_preds
        if self.model_input_image is None or self.idx2label is None:
            raise ValueError("ClassificationResult.plot: needs model_input_image and idx2label")
        exp_logits = np.exp(self.logits) + np.finfo(self.logits.dtype).eps
        probs = exp_logits / np.sum(exp_logits)
        x = self.model_input_image
        image = vz.unnormalize_device((x if x.is_cuda else x.cuda()).to(torch.float32))
        return {"top_probs": plot_top_preds(image, probs, self.idx2label, k=5, target_label=self.target_label)}

    def plot(self) -> dict[str, np.ndarray]:
        from ..keypoints.visualization import to_host
        return {name: to_host(figure) for name, figure in self._plot_device().items()}

    def plot_jpeg(self, quality: int = 90, subsampling="444") -> dict[str, bytes]:
        """plot() as the .jpg file the reference's callbacks save: encoded on the GPU (keypoints/jpeg.py), only the compressed bytes
        copied back."""
        from ..keypoints.jpeg import encode_jpeg_device
        figures = self._plot_device()
        return dict(zip(figures, encode_jpeg_device(list(figures.values()), quality, subsampling)))


class ClassificationModule:
    """eval_dtype: the element type of the inference engine that `validation_step` runs ("bf16" / "fp16").  None (default) leaves the
    net's engine as it is; a name calls `net.set_engine_dtype` once, here.
    max_grad_norm (not in the reference; None = off, the step is exactly the reference's sequence): the gradients are clipped to this
    global norm (grad_norm_type: 2 or inf) between the backward and the step by optim.clip_grad_norm_ -- on the optimizer's device
    table for an optimizer of ..optim, with torch's function for any other -- and metrics["grad_norm"] is the norm before clipping.
    ema_decay (not in the reference; None = off: the step as before, bit for bit, and no "ema" entry in state_dict()): a number keeps
    an exponential moving average of the weights, `self.ema = optim.ModelEMA(net, optimizer, ema_decay, ema_warmup, ema_use_buffers)`,
    updated inside the step launch of an optimizer of ..optim and by ema.update() after any other's.  validation_step runs on the
    averaged weights (ema.applied()); state_dict() / load_state_dict() carry {"ema": ModelEMA.state_dict()}.
    evaluator (not in the reference; None = off, validation_step as before): an `evaluation.ClsEvaluator`; every validation_step also
    adds its batch to it (one more launch pair, nothing read back), so an epoch's per-class accuracy and confusions are one
    `evaluator.result()` away."""

    def __init__(self, model: ClassificationModel, loss_fn: ClassificationLoss, optimizer: torch.optim.Optimizer,
                 idx2label: dict | None = None, eval_dtype: str | None = None, max_grad_norm: float | None = None, grad_norm_type: float = 2.0,
                 ema_decay: float | None = None, ema_warmup: bool = False, ema_use_buffers: bool = False, evaluator=None):
        self.evaluator = evaluator
        self.model, self.loss_fn, self.optimizer, self.idx2label = model, loss_fn, optimizer, idx2label
        self.ema = None if ema_decay is None else ModelEMA(model.net, optimizer, ema_decay, ema_warmup, ema_use_buffers)
        self.max_grad_norm, self.grad_norm_type = max_grad_norm, grad_norm_type
        self.eval_dtype = eval_dtype
        if eval_dtype is not None:
            model._bare().set_engine_dtype(eval_dtype)

    def state_dict(self) -> dict:
        """The module's own checkpoint entries: {"ema": ...} with ema_decay set, nothing otherwise (this module has no scaler)."""
        return {} if self.ema is None else {"ema": self.ema.state_dict()}

    def load_state_dict(self, state_dict: dict) -> None:
        if self.ema is not None:
            self.ema.load_state_dict(state_dict["ema"])

    def batch_to_device(self, batch):
        images, targets = batch
        dev = self.model.device
        return images.to(dev), targets.to(dev, non_blocking=True)

    def training_step(self, batch, batch_idx: int = 0) -> dict[str, float]:
        """module.py:45-57: forward, loss, backward, optimizer step -> {"top-1_error", "top-5_error", "loss"}.  The result record is
        read between the backward and the optimizer step, so a target outside [0, num_classes) raises IndexError before any weight or
        momentum moves (the forward has already updated the BatchNorm running statistics by then, as in the reference, whose loss raises
        after its forward too)."""
        images, targets = batch
        logits = self.model.net(images)
        loss = self.loss_fn.calculate_loss(targets, logits)
        self.optimizer.zero_grad()
        loss.backward()
        metrics = self.loss_fn.metrics()
        if self.max_grad_norm is not None:
            metrics["grad_norm"] = clip_grad_norm_(self.optimizer, self.max_grad_norm, self.grad_norm_type).item()
        self.optimizer.step()
        if self.ema is not None and self.ema.optimizer is None:  # (attached to a device optimizer it was updated inside the step)
            self.ema.update()
        self.model._bare().mark_dirty()
        return metrics

    def validation_step(self, batch, batch_idx: int = 0):
        """module.py:59-82: the eval-mode engine forward, the same loss and metrics, one result record per image."""
        images, targets = batch
        net = self.model._bare()
        was_training = net.training
        net.eval()
        try:
            with torch.no_grad(), (self.ema.applied() if self.ema is not None else contextlib.nullcontext()):
                logits = self.model.net(images)
                self.loss_fn.calculate_loss(targets, logits)
                if self.evaluator is not None:
                    self.evaluator.update(logits, targets)
        finally:
            net.train(was_training)
        metrics = self.loss_fn.metrics()
        lg, tg = logits.detach().cpu().numpy(), targets.detach().cpu().numpy()
        results = []
        for i in range(len(lg)):
            t = int(tg[i])
            results.append(ClassificationResult(lg[i], t, int(np.argmax(lg[i])), self.idx2label[t] if self.idx2label is not None else None,
                                                images[i], self.idx2label))
        return metrics, results
