#!/usr/bin/env python3
"""Time the weight gradients of the classification head's convolutions one by one, at the shapes of a training step (W32, B = 80, 224^2):
HIP events around `iters` back-to-back launches of hh_conv2d_wgrad per layer, with the plan (variant, workers = partial sets, tiles) and
the fp32 partial-sum workspace of each.

  python3 tools/cls_head_wgrad_time.py [--batch 80] [--size 224] [--iters 20] [--only NAME_SUBSTRING] [--out result.json]

Under `rocprofv3 --kernel-trace --stats` with `--only downsample_blocks.2` (or `final_conv`) the statistics split that layer's time into
conv_wgrad_kernel and wgrad_reduce_kernel.  Needs the GPU; prints one JSON line.
"""
import argparse
import ctypes
import importlib
import json
import os
import sys

import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
pkg = importlib.import_module("pytorch-human-pose_amd")
ops = importlib.import_module("pytorch-human-pose_amd.keypoints.train_ops")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=80)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--only", default="")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cls_head_wgrad_time.py needs the GPU: there is nothing to time without one")
    lib = pkg._lib.load()
    net = pkg.ClassificationHRNet(32, 1000)
    head = net.classification_head
    B = a.batch
    rows, total = [], 0.0
    for name, m in head.named_modules():
        if not isinstance(m, nn.Conv2d) or a.only not in name:
            continue
        # the input map of the layer: scale i of the head works at size / 4 / 2^i; a downsample block reads the scale above its output
        parts = name.split(".")
        i = int(parts[1]) if parts[0] != "final_conv" else 3
        hw = a.size // 4 >> i
        cout, cin, ks, _ = m.weight.shape
        stride = m.stride[0]
        plan = (ctypes.c_int * 3)()
        assert lib.hh_conv2d_wgrad_plan(B, hw, hw, cin, cout, ks, stride, plan) == 0, name
        x = torch.randn(B, cin, hw, hw, device="cuda").to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
        dy = torch.randn(B, cout, hw // stride, hw // stride, device="cuda").to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
        for _ in range(3):
            ops.conv2d_weight_grad(x, dy, ks, stride)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            ops.conv2d_weight_grad(x, dy, ks, stride)
        e1.record()
        e1.synchronize()
        ms = e0.elapsed_time(e1) / a.iters
        total += ms
        rows.append(dict(layer=name, cin=cin, cout=cout, ks=ks, stride=stride, hw=hw, variant=plan[0], workers=plan[1], tiles=plan[2],
                         partial_mb=lib.hh_conv2d_wgrad_workspace_bytes(B, hw, hw, cin, cout, ks, stride) / 1e6, ms=ms,
                         tflops=2.0 * B * (hw // stride) ** 2 * cin * cout * ks * ks / (ms * 1e-3) / 1e12))
    line = json.dumps(dict(batch=B, size=a.size, iters=a.iters, head_wgrad_ms_sum=total, layers=rows))
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
