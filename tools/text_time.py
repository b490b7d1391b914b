#!/usr/bin/env python3
"""Time the text labels on the GPU: the text launch alone for the video labels on one 640-high frame and for 32 classifier plots,
`video_frame(labels=...)` beside `video_frame()` and the same pair with `jpeg=`, and `plot_top_preds_batch` of 32 records.

  python3 tools/text_time.py [--iters 50] [--rounds 5] [--out result.json]

Launch times are HIP-event times over `--iters` back-to-back launches on frames, table and tile list already on the device (median
of `--rounds` rounds; the launch draws in place, so the pixels of later iterations differ, the work does not); call times are host
clocks around work that ends in a device synchronise, the two variants of a pair alternated round by round: their difference is what
the labels add.  There is no threshold to meet: the labelled area is small and the launch is latency-bound.  Needs the GPU; prints one
JSON line."""
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
tx = importlib.import_module("pytorch-human-pose_amd.keypoints.text")
cls = importlib.import_module("pytorch-human-pose_amd.classification")
cvz = importlib.import_module("pytorch-human-pose_amd.classification.visualization")


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


def launch_stats(frames, tables, iters, rounds):
    launch = tx.stage_put_txt(frames, tables)
    for _ in range(3):
        launch()
    torch.cuda.synchronize()
    TH, TW, _, _ = tx.text_config()
    return dict(frames=len(frames), primitives=int(sum(len(t) for t in tables)), tiles=launch.num_tiles, all_tiles=int(sum(-(-f.shape[0] // TH) * -(-f.shape[1] // TW) for f in frames)),
                launch_ms=event_ms(launch, iters, rounds))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("text_time.py needs the GPU: there is nothing to time without one")
    dev = "cuda:0"
    res = dict(text_config=list(tx.text_config()), device=torch.cuda.get_device_name(0))
    rs = np.random.RandomState(0)

    # the text launch alone: the video labels on one 640 x 1137 frame (1920 x 1080 at height 640)
    labels = tx.video_labels(17, 300, (512, 896), {"preprocess": 3, "model": 21, "postprocess": 5})
    frame = torch.from_numpy(rs.randint(0, 256, (640, 1137, 3)).astype(np.uint8)).to(dev)
    res["video_labels_launch"] = launch_stats([frame], [tx.video_table(640, 1137, labels)], a.iters, a.rounds)

    # ... and 32 classifier plots of 512 x 683 (a 4:3 image at height 512) with a target box each
    idx2label = {i: f"class number {i}" for i in range(1000)}
    probs = rs.dirichlet(np.ones(1000)).astype(np.float32)
    frames = [torch.from_numpy(rs.randint(0, 256, (512, 683, 3)).astype(np.uint8)).to(dev) for _ in range(32)]
    res["classifier_plots_launch"] = launch_stats(frames, [cvz.top_preds_table(512, 683, probs, idx2label, 5, "class number 3")] * 32, a.iters, a.rounds)

    # plot_top_preds_batch of 32 records against 32 single plot() calls: upload, resizes, one text launch, copy back
    records = [cls.InferenceClassificationResult(rs.randint(0, 256, (375, 500, 3)).astype(np.uint8), np.log(probs), probs, 0, "class number 0", "class number 3", idx2label)
               for _ in range(32)]
    cls.plot_top_preds_batch(records)
    batch, single = pair_ms(lambda: cls.plot_top_preds_batch(records), lambda: [r.plot() for r in records], 3, a.rounds)
    res["plot_top_preds_32"] = dict(raw=[375, 500], batch_call_ms=batch, single_calls_ms=single)

    # video_frame with and without labels, raw frame and jpeg= route
    net = pkg.HigherHRNet(17, 32)
    net.load_state_dict({k: torch.from_numpy(pkg.synth.synth_param(k, v.shape, 3)) for k, v in net.state_dict().items()})
    model = pkg.InferenceKeypointsModel(net.to(dev).eval(), det_thr=0.05, tag_thr=0.5, use_flip=False, input_size=512, device=dev)
    image = rs.randint(0, 256, (1080, 1920, 3)).astype(np.uint8)
    jpeg = dict(quality=90, subsampling="420")
    for _ in range(3):
        model.video_frame(image, labels=labels)
        model.video_frame(image, jpeg=jpeg, labels=labels)
    iters = max(5, a.iters // 5)
    plain, labelled = pair_ms(lambda: model.video_frame(image), lambda: model.video_frame(image, labels=labels), iters, a.rounds)
    jplain, jlabelled = pair_ms(lambda: model.video_frame(image, jpeg=jpeg), lambda: model.video_frame(image, jpeg=jpeg, labels=labels), iters, a.rounds)
    res["video_frame"] = dict(image=[1080, 1920], plain_call_ms=plain, labels_call_ms=labelled, added_ms=labelled[0] - plain[0])
    res["video_frame_jpeg"] = dict(image=[1080, 1920], plain_call_ms=jplain, labels_call_ms=jlabelled, added_ms=jlabelled[0] - jplain[0])
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
