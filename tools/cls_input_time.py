#!/usr/bin/env python3
"""Time the classifier's training input for one batch: the device path (classification/input.py: one pinned copy of uint8 pixels,
descriptors and targets, one hh_resized_crop_u8_batch launch) against the same samples and the same crops through the torch-CPU
pipeline the reference runs in its dataset workers (ToTensor -> crop -> antialiased bilinear resize -> flip -> Normalize; torchvision
is not needed: its tensor resized_crop is F.interpolate(antialias=True) on the cropped tensor) plus the fp32 upload, at B = 80,
224^2, synthetic images of mixed ImageNet-like sizes.

  python3 tools/cls_input_time.py [--batch 80] [--size 224] [--threads 16] [--iters 20] [--rounds 5] [--out result.json]

Host clocks around work that ends in a device synchronise, `--rounds` alternated rounds of `--iters` calls each after warm-up; the
kernel alone is HIP-event time over back-to-back launches on a batch already on the device.  The CPU pipeline runs its images one
after the other with torch's intra-op pool at `--threads` threads (the reference spreads images over worker processes instead; the
single-thread figure is reported next to it, so perfect scaling over 16 workers can be read off as that figure / 16).  JPEG decode
is in neither path.  Needs the GPU; prints one JSON line.
"""
import argparse
import ctypes as C
import importlib
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
pkg = importlib.import_module("pytorch-human-pose_amd")
ci_mod = importlib.import_module("pytorch-human-pose_amd.classification.input")

SIZES = [(375, 500), (500, 375), (333, 500), (500, 333), (480, 640), (600, 800), (256, 341), (1200, 1600)]  # h x w, cycled


def timed_ms(fn, iters):
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts


def stats(ts):
    return dict(median=float(np.median(ts)), min=float(np.min(ts)), max=float(np.max(ts)), n=len(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=80)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cls_input_time.py needs the GPU: there is nothing to time without one")
    dev, B, S = "cuda:0", a.batch, a.size
    rs = np.random.RandomState(0)
    samples = [(rs.randint(0, 256, SIZES[b % len(SIZES)] + (3,)).astype(np.uint8), b % 1000) for b in range(B)]
    torch.manual_seed(0)
    params = [ci_mod.random_resized_crop_params(*s[0].shape[:2]) for s in samples]
    ci = ci_mod.ClsInput(S, device=dev)
    mean, std = torch.tensor(ci.mean)[:, None, None], torch.tensor(ci.std)[:, None, None]

    def cpu_one(img, p):
        x = torch.from_numpy(img).permute(2, 0, 1).float().div(255)
        x = x[:, p.top:p.top + p.height, p.left:p.left + p.width]
        x = F.interpolate(x[None], size=(S, S), mode="bilinear", align_corners=False, antialias=True)[0]
        if p.flip:
            x = x.flip(-1)
        return x.sub(mean).div(std)

    def cpu_batch():
        return torch.stack([cpu_one(s[0], p) for s, p in zip(samples, params)]), torch.tensor([s[1] for s in samples])

    def cpu_path():
        images, targets = cpu_batch()
        return images.to(dev), targets.to(dev, non_blocking=True)

    def device_path():
        return ci.build(samples, params)

    # the two paths must agree before their times are compared (fp32 roundings apart: tests/cls_input_budget.py has the bound)
    torch.set_num_threads(a.threads)
    want, got = cpu_batch()[0], device_path()[0].cpu()
    max_diff = float((want - got).abs().max())
    assert max_diff < 1e-3, f"device and CPU pipelines differ by {max_diff}"

    for fn in (cpu_path, device_path):  # warm-up: pinned staging, allocator, thread pool
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    cpu_rounds, dev_rounds = [], []
    for _ in range(a.rounds):  # alternated
        cpu_rounds.append(stats(timed_ms(cpu_path, max(2, a.iters // 4))))
        dev_rounds.append(stats(timed_ms(device_path, a.iters)))
    torch.set_num_threads(1)
    t0 = time.perf_counter()
    for _ in range(2):
        cpu_batch()
    cpu_1thread_ms = (time.perf_counter() - t0) / 2 * 1e3
    torch.set_num_threads(a.threads)
    cpu_images = cpu_batch()[0]
    upload = stats(timed_ms(lambda: cpu_images.to(dev), a.iters))

    # ---- the kernel alone: the batch already on the device
    lib = pkg._lib.load()
    shapes = [s[0].shape[:2] for s in samples]
    offs, desc_off, target_off, total = ci.layout(shapes)
    host = np.zeros(total, np.uint8)
    descs = host[desc_off:target_off].view(ci_mod._CROP_DESC)
    for b, ((img, _), p) in enumerate(zip(samples, params)):
        host[offs[b]:offs[b + 1]] = img.reshape(-1)
        descs[b] = (int(offs[b]), *shapes[b], p.top, p.left, p.height, p.width, S, S, 0, 0, int(p.flip), 1)
    raw = torch.from_numpy(host).to(dev)
    out = torch.empty((B, 3, S, S), device=dev, dtype=torch.float32)
    fp = C.POINTER(C.c_float)
    stream = torch.cuda.current_stream().cuda_stream

    def kernel():
        pkg._lib.check(lib.hh_resized_crop_u8_batch(raw.data_ptr(), raw.data_ptr() + desc_off, descs.ctypes.data, B, out.data_ptr(), S, S,
                                                    ci.mean.ctypes.data_as(fp), ci.std.ctypes.data_as(fp), stream))

    def event_ms(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            kernel()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / iters

    event_ms(5)
    kernel_runs = [event_ms(a.iters) for _ in range(a.rounds)]
    assert torch.equal(out.cpu(), got)
    crop_bytes = sum(p.height * p.width * 3 for p in params)
    res = dict(batch=B, size=S, threads=a.threads, iters=a.iters, rounds=a.rounds, image_sizes=SIZES, max_abs_diff_between_paths=max_diff,
               device_path_ms_rounds=dev_rounds, cpu_path_ms_rounds=cpu_rounds, cpu_pipeline_1_thread_ms=cpu_1thread_ms,
               cpu_pipeline_1_thread_ms_per_image=cpu_1thread_ms / B, fp32_upload_ms=upload,
               device_h2d_bytes=int(ci.last_h2d_bytes), device_launches=int(ci.last_launches), cpu_h2d_bytes=int(cpu_images.numel() * 4 + 8 * B),
               kernel_ms_runs=kernel_runs, kernel_crop_bytes=int(crop_bytes), kernel_output_bytes=int(out.numel() * 4),
               kernel_gb_per_s=(crop_bytes + out.numel() * 4) / (float(np.median(kernel_runs)) * 1e-3) / 1e9)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
