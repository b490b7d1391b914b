"""ClassificationHRNet with the reference's module interface, executed by the gfx950 HIP engine.

Stands in for `/root/reference/src/classification/architectures/hrnet.py:64-74`
(`ClassificationHRNet(C, num_classes).forward(images) -> logits`), BASELINE.json configs[0].
Same state-dict keys as the reference (backbone with a 4-scale last fusion + classification_head.*).
"""
from __future__ import annotations

import torch
from torch import Tensor

from ... import _lib
from ...keypoints.architectures.higher_hrnet import EngineModule
from ...keypoints.architectures.spec import classification_hrnet_rows


class ClassificationHRNet(EngineModule):
    """`dtype="bf16"` (default) or `"fp16"`: the element type of the inference engine (see HigherHRNet; the classifier has no fp8 form)."""

    def __init__(self, C: int = 32, num_classes: int = 1000, dtype: str = "bf16"):
        super().__init__()
        self.C = C
        self.num_classes = num_classes
        self.stages_C = [C, 2 * C, 4 * C, 8 * C]
        self._init_engine(classification_hrnet_rows(C, num_classes), lambda lib, code: lib.hh_create_classifier(C, num_classes, code), dtype)

    def forward(self, images: Tensor) -> Tensor:
        if self.training:  # batch-stat BatchNorm, differentiable: keypoints/train_net.py on the training kernels (bf16 activations by default)
            from ...keypoints.train_net import classification_hrnet_train_forward
            if not images.is_cuda:
                raise _lib.HHError("ClassificationHRNet forward needs a CUDA/HIP tensor: there is no CPU path")
            self._dirty = True  # parameters / running statistics change under training: re-fold before the next eval forward
            return classification_hrnet_train_forward(self, images)
        x = self._check_input(images)
        B, _, H, W = x.shape
        logits = torch.empty((B, self.num_classes), device=x.device, dtype=torch.float32)
        _lib.launch(x.device, self._lib.hh_forward_classifier, self._h, x.data_ptr(), B, H, W, logits.data_ptr())
        return logits
