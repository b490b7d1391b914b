"""Time the classifier's input built from JPEG files: `ClsInput.build` of `JpegImage` samples (the window decode: only each sample's crop
is turned into pixels) against the parent's route, Pillow's decode of every whole file on the host plus `ClsInput.build` of the arrays.
32 streams of 480 x 640 (the synthetic scene of tools/jpeg_decode_time.py, 4:2:0, quality 90, written by Pillow, no restart markers),
through indexes of one MCU row and of 8 MCUs per segment; once with `RandomResizedCrop` draws from a fixed seed and once with the
inference geometry (Resize(256) + CenterCrop(224): the whole image is the source rectangle).  Both routes in one process on the same
GPU, alternated round by round, after warm-up; medians with the spread (min..max) of the rounds.  The segments and MCUs walked come
from the host twin's counts (derived from the rule, not measured).  Writes its tables into profiles/cls_input_jpeg.md between the two
`cls_input_jpeg_time` marker lines, or into --out as a whole file.

    python tools/cls_input_jpeg_time.py [--rounds 9] [--out FILE]
    python tools/cls_input_jpeg_time.py --kernels-only 20     # only the JpegImage builds (train draws), for a kernel trace around them

Not measured here: route (b) of the issue, whole-image `decode_jpeg_device` followed by a build of the decoded tensors' crops.
`ClsInput.build` stages host arrays, so the decoded pixels would have to come back to the host and cross again: two extra copies that
no user would make.  It is left out.
"""
import argparse
import importlib
import io
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
PKG = "pytorch-human-pose_amd"
H, W, N, S = 480, 640, 32, 224


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernels-only", type=int, default=0)
    args = ap.parse_args()
    from PIL import Image
    from jpeg_decode_time import streams
    importlib.import_module(PKG)
    J = importlib.import_module(PKG + ".keypoints.jpeg")
    inp = importlib.import_module(PKG + ".classification.input")
    data = streams(False)
    items = {"one MCU row": [J.JpegImage(s) for s in data], "8 MCUs": [J.JpegImage(s, J.build_jpeg_index(s, 8)) for s in data]}
    ci = inp.ClsInput(S, device="cuda:0")
    torch.manual_seed(0)
    geometry = {"RandomResizedCrop, seed 0": [inp.random_resized_crop_params(H, W) for _ in range(N)],
                "inference (whole image)": [inp.inference_geometry(H, W, resize=ci.resize, crop=S) for _ in range(N)]}

    def pillow(s):
        return np.array(Image.open(io.BytesIO(s)).convert("RGB"))

    if args.kernels_only:
        params = geometry["RandomResizedCrop, seed 0"]
        for k, v in items.items():
            for _ in range(args.kernels_only):
                ci.build([(it, 0) for it in v], params)
            torch.cuda.synchronize()
            print(k, ci.jpeg_status().tolist().count(0), "of", N, "clean")
        return

    def fmt(ts):
        return f"{statistics.median(ts):.3f} ({min(ts):.3f}..{max(ts):.3f})"

    def alternate(routes: dict) -> dict:
        for fn in routes.values():  # warm up
            fn()
            fn()
        wall = {k: [] for k in routes}
        for _ in range(args.rounds):
            for k, fn in routes.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                wall[k].append((time.perf_counter() - t0) * 1e3)
        return wall

    lines = [f"Measured by tools/cls_input_jpeg_time.py on {torch.cuda.get_device_name(0)}: `ClsInput({S}).build` of {N} samples from {N} streams of {H}x{W} "
             f"(mean {sum(map(len, data)) // N} bytes; the synthetic scene, 4:2:0, quality 90, written by Pillow, no restart markers); {args.rounds} rounds "
             "after warm-up, routes alternated in one process; wall milliseconds per batch, median (min..max), each ending in a device synchronise.  "
             "(a) = Pillow decode of every file on one host core + build of the arrays (the parent's route); (c) = build of prepared `JpegImage` samples.  "
             "Segments and MCUs walked: sums over the batch from the host twin's counts.", "",
             "| geometry | index | (a) Pillow + arrays | of which Pillow | (c) JpegImage | bytes staged (a) | bytes staged (c) | segments walked (of) | MCUs walked | "
             "MCUs stored (of) |", "|---|---|---|---|---|---|---|---|---|---|"]
    for gname, params in geometry.items():
        for iname, its in items.items():
            staged = {}

            def route_a():
                ci.build([(pillow(s), 0) for s in data], params)
                staged["a"] = ci.last_h2d_bytes

            def route_c():
                ci.build([(it, 0) for it in its], params)
                staged["c"] = ci.last_h2d_bytes

            wall = alternate({"a": route_a, "c": route_c})
            assert not ci.jpeg_status().any()
            dec = []
            for _ in range(args.rounds):
                t0 = time.perf_counter()
                for s in data:
                    pillow(s)
                dec.append((time.perf_counter() - t0) * 1e3)
            total = dict(segments_walked=0, mcus_walked=0, mcus_stored=0)
            for it, p in zip(its, params):
                q = ci.window(H, W, p)
                counts = {}
                J.decode_jpeg_host(it.data, index=it.segments, window=(q.top, q.left, q.height, q.width), counts=counts)
                for k in total:
                    total[k] += counts[k]
            nseg, nmcu = sum(len(it.segments) for it in its), N * (H // 16) * (W // 16)
            lines.append(f"| {gname} | {iname} | {fmt(wall['a'])} | {fmt(dec)} | {fmt(wall['c'])} | {staged['a']} | {staged['c']} | {total['segments_walked']} ({nseg}) | "
                         f"{total['mcus_walked']} | {total['mcus_stored']} ({nmcu}) |")
    prep = []
    for _ in range(args.rounds):
        t0 = time.perf_counter()
        [J.JpegImage(s) for s in data]
        prep.append((time.perf_counter() - t0) * 1e3)
    lines += ["", f"Not included in (c): `JpegImage(...)` of the {N} files (parse + index of one MCU row), once per file: {fmt(prep)} ms."]
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out is not None:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
        return
    path = os.path.join(REPO, "profiles", "cls_input_jpeg.md")
    begin, end = "<!-- cls_input_jpeg_time:begin -->\n", "<!-- cls_input_jpeg_time:end -->\n"
    with open(path) as f:
        doc = f.read()
    head, _, rest = doc.partition(begin)
    _, _, tail = rest.partition(end)
    with open(path, "w") as f:
        f.write(head + begin + text + end + tail)


if __name__ == "__main__":
    main()
