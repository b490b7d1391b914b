#!/usr/bin/env python3
"""Time the pose overlay on the GPU: the render and resize launches alone, the overlay stage of a video frame (table, upload, render,
resize to height 640, pinned copy back) and `video_frame` beside `model(image)` at 1920 x 1080, and `infer_images(render=...)` beside
`render=None` at B = 32.

  python3 tools/render_time.py [--iters 30] [--rounds 5] [--batch 32] [--out result.json]

Launch times are HIP-event times over `--iters` back-to-back launches on data already on the device (median of `--rounds` rounds);
call times are host clocks around work that ends in a device synchronise, the two variants of a pair alternated round by round.  The
people of the stage timings are seeded synthetic poses (1, 10, 30 of them, a third of the frame tall); `video_frame` and `model(image)`
run a seeded synthetic net, whose own number of people is reported.  Beside the times: the compulsory traffic of the render launch
(3 bytes read + 3 bytes written per pixel), the share of it that the launch achieves, and the survivors per tile (primitives whose box
meets a tile: the inside tests every pixel of that tile pays for).  Needs the GPU; prints one JSON line."""
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
vz = importlib.import_module("pytorch-human-pose_amd.keypoints.visualization")
LIMBS = pkg.keypoints.model.COCO_LIMBS
H, W = 1080, 1920


def poses(P, seed=0):
    rng = np.random.default_rng(seed + P)
    centre = rng.uniform([100, 250], [W - 100, H - 250], (P, 1, 2))
    return centre + rng.normal(0, [45, 110], (P, 17, 2)), rng.uniform(0.3, 1.0, (P, 17))


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


def pair_ms(fa, fb, iters, rounds):
    """Two call variants alternated round by round -> (median, min, max) of the per-call host time of each."""
    ta, tb = [], []
    for _ in range(rounds):
        for fn, ts in ((fa, ta), (fb, tb)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(iters):
                fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3 / iters)
    return [(float(np.median(t)), float(min(t)), float(max(t))) for t in (ta, tb)]


def direct_launch(frame_dev, table, alpha, bgr):
    """A closure that repeats only hh_render_poses_u8_batch on a descriptor and a table that are already on the device."""
    lib = pkg._lib.load()
    out = torch.empty_like(frame_dev)
    base = min(frame_dev.data_ptr(), out.data_ptr())
    desc = np.zeros(1, vz.DESC)
    w0, w1 = vz.blend_weights(alpha)
    desc[0] = (frame_dev.data_ptr() - base, out.data_ptr() - base, H, W, 0, len(table), w0, w1, vz.FLAG_BGR if bgr else 0, 0)
    table = np.ascontiguousarray(table)
    d_dev = torch.from_numpy(desc.view(np.uint8).copy()).to(frame_dev.device)
    t_dev = torch.from_numpy(table.view(np.uint8).copy()).to(frame_dev.device)
    stream = torch.cuda.current_stream(frame_dev.device).cuda_stream

    def fn():
        pkg._lib.check(lib.hh_render_poses_u8_batch(base, d_dev.data_ptr(), desc.ctypes.data, t_dev.data_ptr(), table.ctypes.data, len(table), 1, stream))
        return out
    return fn


def survivors(table, cfg):
    Th, Tw = cfg[0], cfg[1]
    ty, tx = np.arange(0, H, Th), np.arange(0, W, Tw)
    x0, y0, x1, y1 = (table[k].astype(np.int64) for k in ("x0", "y0", "x1", "y1"))
    meets_x = (x0[:, None] <= np.minimum(tx + Tw, W)[None] - 1) & (x1[:, None] >= tx[None])
    meets_y = (y0[:, None] <= np.minimum(ty + Th, H)[None] - 1) & (y1[:, None] >= ty[None])
    per_tile = (meets_y[:, :, None] & meets_x[:, None, :]).sum(0)
    return dict(mean=float(per_tile.mean()), max=int(per_tile.max()), tiles_with_any=float((per_tile > 0).mean()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("render_time.py needs the GPU: there is nothing to time without one")
    dev = "cuda:0"
    cfg = vz.render_config()
    image = np.random.RandomState(0).randint(0, 256, (H, W, 3)).astype(np.uint8)
    frame_dev = torch.from_numpy(image).to(dev)
    res = dict(frame=[H, W], render_config=list(cfg), compulsory_bytes=6 * H * W, stages={})

    for P in (1, 10, 30):
        coords, scores = poses(P)
        table = vz.build_primitives(coords, scores, LIMBS, 0.05, "limb", vz.DEFAULT_PALETTE, 0.65)

        def stage():
            t = vz.build_primitives(coords, scores, LIMBS, 0.05, "limb", vz.DEFAULT_PALETTE, 0.65)
            f = vz.render_frames_device([frame_dev], [t], 0.65, bgr=True)[0]
            return vz.to_host(vz.resize_device(f, int(640 * W / H), 640))

        launch_only = direct_launch(frame_dev, table, 0.65, True)

        drawn = launch_only()

        def resize_only():
            return vz.resize_device(drawn, int(640 * W / H), 640)

        for fn in (stage, launch_only, resize_only):
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        render = event_ms(launch_only, a.iters, a.rounds)
        resize = event_ms(resize_only, a.iters, a.rounds)
        whole = pair_ms(stage, stage, a.iters, a.rounds)[0]
        res["stages"][str(P)] = dict(primitives=int(len(table)), survivors_per_tile=survivors(table, cfg), render_launch_ms=render, resize_launch_ms=resize,
                                     overlay_stage_call_ms=whole, achieved_GBps=6 * H * W / (render[0] * 1e-3) / 1e9)

    net = pkg.HigherHRNet(17, 32)
    net.load_state_dict({k: torch.from_numpy(pkg.synth.synth_param(k, v.shape, 3)) for k, v in net.state_dict().items()})
    model = pkg.InferenceKeypointsModel(net.to(dev).eval(), det_thr=0.05, tag_thr=0.5, use_flip=False, input_size=512, device=dev)
    for _ in range(3):
        r, _f = model.video_frame(image)
        model(image, None)
    plain, video = pair_ms(lambda: model(image, None), lambda: model.video_frame(image), max(5, a.iters // 3), a.rounds)
    res["video_frame"] = dict(people=int(len(r.kpts_coords)), model_call_ms=plain, video_frame_call_ms=video)

    rs = np.random.RandomState(1)
    images = [rs.randint(0, 256, (480, 640, 3)).astype(np.uint8) for _ in range(a.batch)]
    opts = dict(color_mode="limb", alpha=0.65)
    for _ in range(2):
        out = model.infer_images(images, max_batch=a.batch, render=opts)
        model.infer_images(images, max_batch=a.batch)
    none, drawn_ms = pair_ms(lambda: model.infer_images(images, max_batch=a.batch), lambda: model.infer_images(images, max_batch=a.batch, render=opts), 3, a.rounds)
    res["infer_images"] = dict(batch=a.batch, image=[480, 640], people=int(sum(len(o.kpts_coords) for o in out)), render_none_ms=none, render_ms=drawn_ms)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
