"""Drop-in for `src/classification/loss.py`: the same class and call signature on the fused softmax cross-entropy kernel.

`hh_softmax_xent` computes the mean loss, its gradient and the top-1 / top-5 hit counts in one launch; the loss is a 0-dim tensor
that takes part in torch autograd, `backward` only scales the stored gradient.  The 16-byte result record of the last call stays on
the device (`ClassificationLoss.last_result`) until somebody reads it: `metrics()` is that one device -> host copy, and it raises if
a target was outside [0, num_classes).  There is no CPU path.

Tie rule of the hit counts (include/hhrnet.h): rank = #{j : z_j > z_t} + #{j < t : z_j == z_t}, hit-k means rank < k -- equal
logits go to the lower index.  `torch.topk`, which the reference's metrics use, leaves the order of equal values unspecified.
"""
from __future__ import annotations

import torch
from torch import Tensor
from torch.nn.modules.loss import _Loss

from .. import _lib
from ..keypoints import train_ops as ops


class _XentFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits: Tensor, targets: Tensor):
        result, grad = ops.softmax_xent(logits, targets, want_grad=ctx.needs_input_grad[0])
        ctx.grad, ctx.dtype = grad, logits.dtype
        ctx.mark_non_differentiable(result)
        return result[:1].view(torch.float32).clone().reshape(()), result  # (a copy: autograd outputs must not alias each other)

    @staticmethod
    def backward(ctx, g: Tensor, _):
        return (ctx.grad * g).to(ctx.dtype), None


class ClassificationLoss(_Loss):
    """classification/loss.py:5-11 (nn.CrossEntropyLoss defaults: mean over the batch, no label smoothing)"""

    def __init__(self) -> None:
        super().__init__()
        self.last_result: Tensor | None = None  # hh_xent_result of the last calculate_loss, on the device
        self._last_batch = 0

    def calculate_loss(self, targets: Tensor, logits: Tensor) -> Tensor:
        if not logits.is_cuda:
            raise _lib.HHError("logits must be a CUDA/HIP tensor: there is no CPU path")
        loss, result = _XentFn.apply(logits, targets)
        self.last_result, self._last_batch = result, logits.shape[0]
        return loss

    def metrics(self) -> dict[str, float]:
        """{"loss", "top-1_error", "top-5_error"} of the last calculate_loss (classification/module.py:15-22,56), one device -> host read."""
        if self.last_result is None:
            raise RuntimeError("ClassificationLoss.metrics: calculate_loss has not run")
        return ops.read_xent_result(self.last_result, self._last_batch)
