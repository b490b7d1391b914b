#!/usr/bin/env python3
"""Time the dataset sample figures on the GPU: the overlay launch alone on 32 frames of 480 x 640 with ten 60-vertex polygons each, and
`plot_examples` of 7 samples at out_size 512.

  python3 tools/sample_plot_time.py [--iters 50] [--rounds 7] [--out result.json]

The launch time is a HIP-event time over `--iters` back-to-back launches on frames and tables already on the device, after 3 warm-up
launches (median, min and max of `--rounds` rounds; out of place, so every launch does the same work).  Its achieved bytes per second
count the 6 bytes per pixel the launch must move (3 read, 3 written), not the tables.  The figure time is a host clock around the
call, which ends in the copy back of the finished figure (a device synchronise); its launches are counted by a wrapper round
_lib.launch.  There is no threshold to meet.  Needs the GPU; prints one JSON line."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
pkg = importlib.import_module("pytorch-human-pose_amd")
sp = importlib.import_module("pytorch-human-pose_amd.keypoints.sample_plot")
_lib = importlib.import_module("pytorch-human-pose_amd._lib")


def event_ms(fn, iters, rounds):
    out = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / iters)
    return float(np.median(out)), float(min(out)), float(max(out))


def blob(rs, h, w, k):
    """A star-shaped polygon of k vertices around a random centre."""
    cx, cy = rs.uniform(0.2 * w, 0.8 * w), rs.uniform(0.2 * h, 0.8 * h)
    ang, rad = np.sort(rs.uniform(0, 2 * np.pi, k)), rs.uniform(0.08, 0.3, k) * min(h, w)
    return np.stack([cx + rad * np.cos(ang), cy + rad * np.sin(ang)], 1).reshape(-1).tolist()


def person(rs, h, w, k=60):
    kpts = np.stack([rs.uniform(0.1 * w, 0.9 * w, 17), rs.uniform(0.1 * h, 0.9 * h, 17), np.full(17, 2.0)], 1)
    return {"segmentation": [blob(rs, h, w, k)], "keypoints": kpts.reshape(-1).tolist(), "iscrowd": 0, "num_keypoints": 17}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sample_plot_time.py needs the GPU: there is nothing to time without one")
    dev = "cuda:0"
    res = dict(overlay_config=list(sp.overlay_config()), device=torch.cuda.get_device_name(0))
    rs = np.random.RandomState(0)

    # the overlay launch alone: 32 frames of 480 x 640, ten 60-vertex polygons each
    n, h, w = 32, 480, 640
    frames = [torch.from_numpy(rs.randint(0, 256, (h, w, 3)).astype(np.uint8)).to(dev) for _ in range(n)]
    tables = [sp.seg_tables([person(rs, h, w) for _ in range(10)], h, w) for _ in range(n)]
    launch = sp.stage_overlay(frames, tables)
    for _ in range(3):
        launch()
    torch.cuda.synchronize()
    ms = event_ms(launch, a.iters, a.rounds)
    moved = 6 * n * h * w
    res["overlay_launch"] = dict(frames=n, size=[h, w], shapes=launch.num_shapes, toggles=launch.num_toggles, launch_ms=ms, bytes_moved=moved,
                                 achieved_gb_per_s=moved / (ms[0] * 1e-3) / 1e9)
    empty = sp.stage_overlay(frames, [(np.zeros((0, 8), np.int32), np.zeros(0, np.uint32))] * n)
    for _ in range(3):
        empty()
    ems = event_ms(empty, a.iters, a.rounds)
    res["overlay_launch_no_shapes"] = dict(launch_ms=ems, achieved_gb_per_s=moved / (ems[0] * 1e-3) / 1e9)

    # plot_examples of 7 samples through TrainInput at out_size 512
    ti = pkg.keypoints.TrainInput(512, [1 / 4, 1 / 2], device=dev)
    annotated = [(rs.randint(0, 256, (h, w, 3)).astype(np.uint8), [person(rs, h, w) for _ in range(4)]) for _ in range(7)]
    params = [ti.inference.draw(h, w) for _ in annotated]
    count = [0]
    real = _lib.launch

    def counting(*args):
        count[0] += 1
        return real(*args)

    fig = ti.plot_examples(annotated, params)  # warm-up
    _lib.launch = counting
    ti.plot_examples(annotated, params)
    _lib.launch = real
    times = []
    for _ in range(a.rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ti.plot_examples(annotated, params)
        times.append((time.perf_counter() - t0) * 1e3)
    res["plot_examples_7"] = dict(out_size=512, raw=[h, w], figure=list(fig.shape), launches=count[0], call_ms=[float(np.median(times)), float(min(times)), float(max(times))])
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
