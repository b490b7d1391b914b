"""Model wrappers of the classifier: the trainer-facing `ClassificationModel` (`src/classification/model.py:12-31`) and the
`InferenceClassificationModel` of `src/classification/model.py:34-72`.
Device placement, DistributedDataParallel / SyncBatchNorm, checkpoints and the example input are keypoints/model.py's BaseModel."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch
from torch import nn

from ..keypoints import jpeg as jp
from ..keypoints.model import BaseModel, checkpoint_weights, parse_checkpoint
from .input import ClsInput, inference_geometry


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


@dataclass
class InferenceClassificationResult:
    """classification/results.py:39-82: one image's logits, their softmax, the prediction (the arg-max, the lower index on a tie, as
    `ClassificationResult` has it), its label, the target label and the label table that `plot()` reads."""
    raw_image: np.ndarray
    logits: np.ndarray
    probs: np.ndarray
    prediction: int
    pred_label: int | str
    target_label: int | str | None = None
    idx2label: dict | None = None

    def plot(self) -> dict[str, np.ndarray]:
        """results.py:70-82: the raw image resized to height 512 (hh_resize_u8) with the five best "{p:.3f}:  {label}" lines and, with
        a target, the green "Target:" box, drawn by one text launch -> {"top_preds": uint8 [512,w,3]}.  For a list of records,
        `classification.plot_top_preds_batch` does the same in one upload, one text launch and one copy back."""
        from .visualization import plot_top_preds_batch
        return {"top_preds": plot_top_preds_batch([self])[0]}

    def plot_jpeg(self, quality: int = 90, subsampling="444") -> dict[str, bytes]:
        """plot() as a .jpg file: drawn and encoded on the GPU (keypoints/jpeg.py); only the compressed bytes are copied back."""
        from ..keypoints.jpeg import encode_jpeg_device
        from .visualization import plot_top_preds_device
        return {"top_preds": encode_jpeg_device(plot_top_preds_device([self]), quality, subsampling)[0]}


class InferenceClassificationModel:
    """`InferenceClassificationModel(net, idx2label, input_size, device, ckpt_path)` of classification/model.py:34-72.  Its transform
    is ToTensor -> Resize(input_size) -> CenterCrop(input_size) -> Normalize; here one hh_resized_crop_u8_batch launch per batch of
    raw images.  `antialias`: torchvision's `T.Resize` default for tensors changed between versions (off before 0.17, on since),
    and the reference does not pass it, so it is an argument here (default: the current torchvision's behaviour)."""

    def __init__(self, net: nn.Module, idx2label: dict, input_size: int = 256, device: str = "cuda:0", ckpt_path: str | None = None,
                 antialias: bool = True):
        self.net = net.to(device)
        self.net.eval()
        self.device, self.input_size, self.idx2label = device, input_size, idx2label
        self._input = ClsInput(input_size, device=device, antialias=antialias)
        if ckpt_path is not None:
            self.load_checkpoint(ckpt_path)

    def load_checkpoint(self, ckpt_path: str, use_ema: bool = False) -> None:
        """base/model.py:167-175: a trainer checkpoint keeps the weights under ["module"]["model"]; a bare state dict is loaded as
        it is.  use_ema=True loads the averaged weights under ["module"]["ema"]["model"] instead (KeyError where there are none)."""
        ckpt = torch.load(ckpt_path, map_location="cpu")
        self.net.load_state_dict(parse_checkpoint(checkpoint_weights(ckpt, use_ema)))

    def prepare_inputs(self, images: list) -> torch.Tensor:
        """[uint8 HWC image] -> [B,3,input_size,input_size] on the device: Resize(input_size) + CenterCrop(input_size) + Normalize.
        An image may also be a `jpeg.JpegImage` or the raw `bytes` of a JPEG file: its pixels are then formed on the device by the
        batch's one window-decode call (`ClsInput.build`).  A stream the decoder does not take (progressive, CMYK, ...) raises by name
        here; pass such a file as a Pillow array in the same batch."""
        size = self.input_size
        images = [jp.JpegImage(im) if isinstance(im, (bytes, bytearray, memoryview)) else im for im in images]
        geometry = [inference_geometry(im.shape[0], im.shape[1], resize=size, crop=size) for im in images]
        return self._input.build([(im, 0) for im in images], geometry)[0]

    def prepare_input(self, image: np.ndarray) -> torch.Tensor:
        """model.py:54-57 -> [1,3,input_size,input_size]."""
        return self.prepare_inputs([image])

    def _records(self, images: list, logits: torch.Tensor, target_labels) -> list:
        lg = logits.cpu().numpy()
        out = []
        for i, im in enumerate(images):
            e = np.exp(lg[i] - lg[i].max())
            pred = int(np.argmax(lg[i]))  # the first maximum: the lower index on a tie
            out.append(InferenceClassificationResult(im, lg[i], e / e.sum(), pred, self.idx2label[pred],
                                                     None if target_labels is None else target_labels[i], self.idx2label))
        return out

    def infer_images(self, raw_images: list, target_labels: list | None = None, max_batch: int = 32) -> list:
        """One record per image, in order, from batches of up to `max_batch` images of any sizes (one input launch + one engine
        forward per batch): what `__call__` returns for each.  An image may be a uint8 array, a `jpeg.JpegImage` or a JPEG file's
        `bytes` (three more launches per batch that holds one); a record's `raw_image` is what was passed."""
        if target_labels is not None and len(target_labels) != len(raw_images):
            raise ValueError("infer_images: one target label per image")
        out = []
        for i in range(0, len(raw_images), max_batch):
            chunk = raw_images[i:i + max_batch]
            with torch.no_grad():
                logits = self.net(self.prepare_inputs(chunk))
            out += self._records(chunk, logits, None if target_labels is None else target_labels[i:i + max_batch])
        return out

    def infer_topk(self, raw_images: list, target_labels: list | None = None, k: int = 5, max_batch: int = 32) -> list:
        """One light record (`evaluation.ClsTopK`) per image, in order: the k best classes, their probabilities and labels and, with a
        target, its rank, picked on the device by hh_cls_score_batch behind each batch's forward: 2k + 1 numbers per image are copied
        back instead of the N logits (and no softmax runs on the host).  Images as for `infer_images`."""
        from .evaluation import infer_topk
        return infer_topk(self, raw_images, target_labels, k, max_batch)

    def __call__(self, raw_image, target_label: int | str | None = None) -> InferenceClassificationResult:
        return self.infer_images([raw_image], [target_label])[0]
