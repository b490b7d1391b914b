#!/usr/bin/env python3
"""Time one ClassificationHRNet training step on the HIP training kernels: forward, fused cross-entropy, backward, SGD(nesterov) step,
at W32, B = 80, 224^2 (the reference's experiments/classification/hrnet_32.yaml batch), bf16 activations.

  python3 tools/cls_train_time.py [--batch 80] [--size 224] [--steps 20] [--warmup 5] [--optimizer torch|hip] [--max-grad-norm X]
                                 [--out result.json]

--optimizer hip: the one-launch SGD of pytorch-human-pose_amd/optim.py instead of torch.optim.SGD (default).
--max-grad-norm X: ClassificationModule(max_grad_norm=X): the gradients are clipped to global norm X before the step (on the device
table for --optimizer hip, with torch's function for torch); last_metrics then holds grad_norm.

The timed window is `steps` training steps behind `warmup` untimed ones, a host clock around work that ends in a device synchronise;
run it with the profiler off.  For kernel time per family run the same command with `--steps 3 --warmup 2` under
`rocprofv3 --kernel-trace --stats` in a call of its own.  The FLOP rate is a WHOLE-STEP figure: 3 x the inference engine's forward FLOPs
per image (hh_forward_flops; forward + data gradient + weight gradient) over the step time, optimizer and launch gaps included.
Needs the GPU; prints one JSON line.
"""
import argparse
import importlib
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
pkg = importlib.import_module("pytorch-human-pose_amd")
cls = importlib.import_module("pytorch-human-pose_amd.classification")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=80)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--optimizer", choices=("torch", "hip"), default="torch")
    ap.add_argument("--max-grad-norm", type=float, default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cls_train_time.py needs the GPU: there is nothing to time without one")
    B, S = a.batch, a.size
    torch.manual_seed(0)
    net = pkg.ClassificationHRNet(32, 1000)
    flops_fwd = net.forward_flops(1, S, S)
    model = cls.ClassificationModel(net)
    model.init_weights()
    model.to_CUDA(0)
    model.net.train()
    opt = (pkg.optim.SGD if a.optimizer == "hip" else torch.optim.SGD)(model.net.parameters(), lr=0.01, momentum=0.9, nesterov=True, weight_decay=1e-4)
    module = cls.ClassificationModule(model, cls.ClassificationLoss(), opt, max_grad_norm=a.max_grad_norm)
    g = torch.Generator().manual_seed(1)
    batch = module.batch_to_device((torch.from_numpy(pkg.synth.synth_images(B, S, S, 0)), torch.randint(0, 1000, (B,), generator=g)))
    for _ in range(a.warmup):
        m = module.training_step(batch)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        m = module.training_step(batch)  # (reads the 16-byte result record: one synchronising copy per step, as a trainer would)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / a.steps * 1e3
    res = dict(optimizer=a.optimizer, max_grad_norm=a.max_grad_norm, batch=B, size=S, steps=a.steps, warmup=a.warmup, precision=net.train_precision, ms_per_step=ms, img_per_s=B / ms * 1e3,
               forward_gflop_per_image=flops_fwd / 1e9, whole_step_tflops=3 * flops_fwd * B / (ms * 1e-3) / 1e12, last_metrics=m,
               peak_memory_gb=torch.cuda.max_memory_allocated() / 2 ** 30)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
