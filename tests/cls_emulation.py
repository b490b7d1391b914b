"""A CPU emulation of the 16-bit storage of the classifier's training step (a plain module for tests/test_gpu_cls_train.py; it never
touches the engine): the reference's layer graph in torch fp32 over a state dict, with every tensor the training kernels STORE in bf16
rounded to bf16 where they store it -- every conv output, every BatchNorm (+ residual, + ReLU) output, every fusion sum, the head's sums
-- and, on the way back, the gradient with respect to each of those tensors rounded to bf16 as well (the kernels store their data
gradients in bf16).  Parameters, their gradients, the pooled features, the Linear and the loss stay fp32, as in the engine.

It models storage precision only, one rounding per stored tensor and direction; accumulation order, the double sums of the BatchNorm
statistics and the packed bf16 weights' own rounding (emulated: weights are rounded to bf16 before each conv) are what the kernels do.
How far this emulation's loss, logits and gradients sit from the fp32 reference is what bf16 storage alone costs on this net and batch.

`python tests/cls_emulation.py` prints its deviation from tests/golden/cls_train_step.npz and from the fp32 oracle's gradients, the
figures recorded as EMULATION_DEVIATION (12 s on 16 CPU threads; tests/test_cls_emulation_cpu.py holds the record against a fresh run):
the cross-entropy of a thousand nearly equal logits hands back a gradient of 1 / 8 at the target and 1e-4 elsewhere, and that signal
crosses ~130 conv + BN layers in bf16, so gradient norms move by up to 25 % and directions to a cosine of 0.76 from storage alone --
against 10 % / 0.92 for HigherHRNet's dense squared-output loss on the same images.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

EPS = 1e-5
# this emulation against the golden (norm ratios) and the fp32 oracle's full gradients (cosines), the four silent conv biases left out
EMULATION_DEVIATION = {"loss_rel": 1.1e-4, "logits": 0.0311, "ratio_min": 0.745, "ratio_max": 1.224, "ratio_median": 0.9959, "cos_min": 0.758,
                       "cos_median": 0.9035}
# max |running statistic after the step - the golden's| of this emulation (momentum 0.1, so a tenth of the batch statistic's distance)
EMULATION_STAT_DISTANCE = {"backbone.bn1.running_mean": 6.26e-6, "classification_head.downsample_blocks.0.1.running_mean": 5.49e-4,
                           "classification_head.final_conv.1.running_var": 1.082e-2}
SEED_W, SEED_X = 11, 1  # the synthetic weights and images of tools/make_golden.py cls_train


class _Q(torch.autograd.Function):
    """round to bf16, forwards and backwards"""

    @staticmethod
    def forward(ctx, x):
        return x.to(torch.bfloat16).float()

    @staticmethod
    def backward(ctx, g):
        return g.to(torch.bfloat16).float()


q = _Q.apply


def _conv(x, sd, name, stride=1):
    w = sd[name + ".weight"]
    wq = w + (w.to(torch.bfloat16).float() - w).detach()  # the packed weights' bf16 values; the gradient reaches the fp32 parameter
    return q(F.conv2d(x, wq, None, stride, (w.shape[-1] - 1) // 2))


STAT_KEYS = ("backbone.bn1.running_mean", "classification_head.downsample_blocks.0.1.running_mean", "classification_head.final_conv.1.running_var")
_RECORD = None  # a dict while measure() runs: {running statistic of STAT_KEYS: its value after this forward, momentum 0.1}


def _bn(x, sd, name, relu=False, res=None, bias=None):
    """bias: the conv bias that x carries in the reference and not here; it only moves the recorded batch mean"""
    if _RECORD is not None:
        with torch.no_grad():
            n = x.numel() // x.shape[1]
            for stat, batch in (("running_mean", x.mean((0, 2, 3)) + (bias if bias is not None else 0)), ("running_var", x.var((0, 2, 3), unbiased=True))):
                if f"{name}.{stat}" in STAT_KEYS:
                    assert n > 1
                    _RECORD[f"{name}.{stat}"] = 0.9 * sd[f"{name}.{stat}"] + 0.1 * batch
    y = F.batch_norm(x, None, None, sd[name + ".weight"], sd[name + ".bias"], True, 0.0, EPS)
    if res is not None:
        y = y + res
    return q(F.relu(y) if relu else y)


def _bottleneck(x, sd, p):
    y = _bn(_conv(x, sd, p + "conv1"), sd, p + "bn1", relu=True)
    y = _bn(_conv(y, sd, p + "conv2"), sd, p + "bn2", relu=True)
    r = _bn(_conv(x, sd, p + "downsample.0"), sd, p + "downsample.1") if p + "downsample.0.weight" in sd else x
    return _bn(_conv(y, sd, p + "conv3"), sd, p + "bn3", relu=True, res=r)


def _basic(x, sd, p):
    y = _bn(_conv(x, sd, p + "conv1"), sd, p + "bn1", relu=True)
    return _bn(_conv(y, sd, p + "conv2"), sd, p + "bn2", relu=True, res=x)


def _fusion(xs, sd, p, n_out):
    outs = []
    for i in range(n_out):
        acc = 0
        for j, x in enumerate(xs):
            qn = f"{p}scales_fusion_layers.{i}.{j}."
            if j == i:
                t = x
            elif j > i:
                t = F.interpolate(_bn(_conv(x, sd, qn + "0"), sd, qn + "1"), scale_factor=2 ** (j - i), mode="nearest")
            else:
                t = x
                for k in range(i - j):
                    t = _bn(_conv(t, sd, f"{qn}{k}.0", 2), sd, f"{qn}{k}.1", relu=(k != i - j - 1))
            acc = acc + t
        outs.append(q(F.relu(acc)))
    return outs


def classification_hrnet_bf16_storage(images: torch.Tensor, sd: dict) -> torch.Tensor:
    """-> logits fp32 [B, N] of the net in .train() mode (batch statistics), differentiable w.r.t. the tensors of `sd`"""
    p = "backbone."
    x = _bn(_conv(q(images), sd, p + "conv1", 2), sd, p + "bn1", relu=True)
    x = _bn(_conv(x, sd, p + "conv2", 2), sd, p + "bn2", relu=True)
    xs = [x]
    for s, nb in enumerate([1, 1, 4, 3]):
        sp = f"{p}stages.{s}."
        for b in range(nb):
            xs = [_chain(t, sd, f"{sp}blocks.{2 * b}.scales_blocks.{i}.", _bottleneck if s == 0 else _basic) for i, t in enumerate(xs)]
            if s > 0:
                xs = _fusion(xs, sd, f"{sp}blocks.{2 * b + 1}.", len(xs))
        if s < 3:
            tp = f"{sp}transition_layer.transition_blocks."
            n = len(xs)
            new = _bn(_conv(xs[-1], sd, f"{tp}{n}.0", 2), sd, f"{tp}{n}.1", relu=True)
            if s == 0:
                xs = [_bn(_conv(xs[0], sd, tp + "0.0"), sd, tp + "0.1", relu=True)]
            xs = xs + [new]
    h = "classification_head."
    out = _bottleneck(xs[0], sd, h + "chann_incr_blocks.0.")
    for i in range(3):
        d = f"{h}downsample_blocks.{i}."
        # (the conv bias in front of a batch-statistics BatchNorm cancels; it is added so that its parameter takes part in the graph)
        down = _bn(_conv(out, sd, d + "0", 2) + sd[d + "0.bias"].view(1, -1, 1, 1) * 0, sd, d + "1", relu=True, bias=sd[d + "0.bias"])
        out = q(_bottleneck(xs[i + 1], sd, f"{h}chann_incr_blocks.{i + 1}.") + down)
    f = h + "final_conv."
    out = _bn(_conv(out, sd, f + "0") + sd[f + "0.bias"].view(1, -1, 1, 1) * 0, sd, f + "1", relu=True, bias=sd[f + "0.bias"])
    return F.linear(out.mean((2, 3)), sd[h + "classifier.weight"], sd[h + "classifier.bias"])


def _chain(t, sd, p, unit):
    for u in range(4):
        t = unit(t, sd, f"{p}{u}.")
    return t


def deviation_stats(grads: dict, ref_grads: dict, ref_norms: dict, names: list) -> dict:
    """-> {ratio_min, ratio_max, ratio_median, cos_min, cos_median} of `grads` against the reference's gradient norms and full gradients"""
    import numpy as np
    ratios = np.array([grads[n].double().norm().item() / max(ref_norms[n], 1e-30) for n in names])
    cos = np.array([float(torch.dot(grads[n].flatten().float(), ref_grads[n].flatten()) / (grads[n].float().norm() * ref_grads[n].norm() + 1e-30)) for n in names])
    return {"ratio_min": float(ratios.min()), "ratio_max": float(ratios.max()), "ratio_median": float(np.median(ratios)),
            "cos_min": float(cos.min()), "cos_median": float(np.median(cos)), "ratios": ratios, "cos": cos}


def measure() -> dict:
    """the emulation and the fp32 oracle on the golden's inputs -> the figures of EMULATION_DEVIATION (and the per-parameter arrays)"""
    import importlib
    import os
    import numpy as np
    from conftest import GOLDEN, PKG
    from oracle import forward as ofw
    pkg = importlib.import_module(PKG)
    g = np.load(os.path.join(GOLDEN, "cls_train_step.npz"))
    net = pkg.ClassificationHRNet(32, 1000)
    sd = {k: torch.from_numpy(pkg.synth.synth_param(k, v.shape, SEED_W)) for k, v in net.state_dict().items()}
    pnames = [n for n, _ in net.named_parameters()]
    x, t = torch.from_numpy(pkg.synth.synth_images(8, 128, 128, seed=SEED_X)), torch.from_numpy(g["targets"])

    def run(fn):
        osd = {k: (v.clone().float().requires_grad_() if k in pnames else v.clone()) for k, v in sd.items()}
        logits = fn(x, osd)
        loss = F.cross_entropy(logits, t)
        loss.backward()
        return logits.detach(), loss.item(), {k: osd[k].grad for k in pnames}
    ofw._TRAIN = True
    try:
        _, _, ograds = run(ofw._classification_hrnet)
    finally:
        ofw._TRAIN = False
    global _RECORD
    _RECORD = {}
    try:
        logits, loss, grads = run(classification_hrnet_bf16_storage)
        stats = dict(_RECORD)
    finally:
        _RECORD = None
    names = [str(n) for n in g["grad.names"]]
    checked = [n for n in names if not (n.endswith(".0.bias") and ("downsample_blocks" in n or "final_conv" in n))]
    out = deviation_stats(grads, ograds, dict(zip(names, g["grad.norms"])), checked)
    out["loss_rel"] = abs(loss - float(g["loss"])) / float(g["loss"])
    out["logits"] = float(np.abs(logits.numpy() - g["logits"]).max() / np.abs(g["logits"]).max())
    out["stat_distance"] = {k: float(np.abs(stats[k].numpy() - g["stat." + k]).max()) for k in STAT_KEYS}
    return out


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    torch.set_num_threads(16)
    print({k: (round(v, 5) if isinstance(v, float) else v) for k, v in measure().items() if not hasattr(v, "shape")})
