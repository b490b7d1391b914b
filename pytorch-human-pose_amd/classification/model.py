"""Trainer-facing model wrapper of the classifier: stands in for `src/classification/model.py:12-31` (`ClassificationModel`).
Device placement, DistributedDataParallel / SyncBatchNorm, checkpoints and the example input are keypoints/model.py's BaseModel."""
from __future__ import annotations

from torch import nn

from ..keypoints.model import BaseModel


class ClassificationModel(BaseModel):
    EXAMPLE_SIZE = 224  # classification/model.py:30-31

    def __init__(self, net: nn.Module):
        super().__init__(net, ["images"], ["logits"])

    def init_weights(self) -> None:
        """classification/model.py:16-23: conv weights ~ kaiming_normal(fan_out, relu), BatchNorm weight 1 / bias 0 (conv biases and
        the Linear keep their constructor's initialisation, as in the reference)."""
        net = self._bare()
        for m in net.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)
        net.mark_dirty()
