#!/usr/bin/env python3
"""Times the classifier's evaluation tail (hh_cls_score_batch; classification/evaluation.py) on the GPU.

  python3 tools/cls_eval_time.py [--images 512] [--batch 32] [--rounds 7] [--out FILE.json]
  rocprofv3 --kernel-trace --stats -d DIR -- python3 tools/cls_eval_time.py --kernels B CONFUSION      (a run of its own per shape)

1. The call alone, N = 1000, k = 5, B = 32 and 256, with and without the confusion matrix: device-event time per hh_cls_score_batch call
   (both launches) over windows of 200 calls and the host's wall time per call (what the enqueueing thread pays), next to
   hh_softmax_xent without its gradient on the same logits.  `--kernels B CONFUSION` only runs 200 calls of each at one shape, for the
   kernel trace: per-kernel times come from that run's statistics, not from here.
2. Images per second: evaluate_images over `images` synthetic 480 x 640 images (W32 net, synthetic weights, input 256), from arrays
   and from JPEG bytes, against the way to the same figures without this module: infer_images, then the numpy / torch restatement of
   the rule (tests/cls_score_ref.py) on the copied-back logits.  The modes alternate within every round; wall time per pass with a
   device synchronise at its end; median and min .. max over the rounds.  The baseline is split into its two parts.  The two paths'
   counts are compared.  Nothing is judged: the claim is only that the new path reads back O(k) numbers per image, or nothing."""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
pkg = importlib.import_module("pytorch-human-pose_amd")
cls = importlib.import_module("pytorch-human-pose_amd.classification")
ops = importlib.import_module("pytorch-human-pose_amd.keypoints.train_ops")
DEV = "cuda:0"
N, K = 1000, 5


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def _batch(B):
    g = torch.Generator().manual_seed(B)
    return (torch.randn(B, N, generator=g) * 3).to(DEV), torch.randint(0, N, (B,), generator=g).to(DEV)


def kernels_only(B, confusion, calls=200):
    z, t = _batch(B)
    ev = cls.ClsEvaluator(N, K, bool(confusion), DEV)
    for _ in range(calls):
        ev.update(z, t)
    for _ in range(calls):
        ops.softmax_xent(z, t, want_grad=False)
    torch.cuda.synchronize()
    print(f"kernels_only: B {B} confusion {confusion}: {calls} calls each, rows {ev.result()['n']}")


def call_time(B, confusion, rounds, n=200):
    z, t = _batch(B)
    ev = cls.ClsEvaluator(N, K, confusion, DEV)
    out = {}
    for name, call in (("cls_score_batch", lambda: ev.update(z, t)), ("softmax_xent_no_grad", lambda: ops.softmax_xent(z, t, want_grad=False))):
        for _ in range(20):
            call()
        torch.cuda.synchronize()
        dev_us, host_us = [], []
        for _ in range(rounds):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            a.record()
            for _ in range(n):
                call()
            b.record()
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            dev_us.append(a.elapsed_time(b) * 1e3 / n)
            host_us.append((t1 - t0) * 1e6 / n)
        out[name] = {"device_us_per_call": spread(dev_us), "host_enqueue_us_per_call": spread(host_us)}
    return {"B": B, "N": N, "k": K, "confusion": confusion, **out}


def synthetic_images(n, seed=0):
    """480 x 640 uint8: a coarse random pattern blown up 8 x, plus a little noise (photographs are smooth; pure noise is no JPEG)"""
    rs = np.random.RandomState(seed)
    out = []
    for _ in range(n):
        coarse = rs.randint(0, 256, (60, 80, 3)).astype(np.int16)
        out.append(np.clip(np.kron(coarse, np.ones((8, 8, 1), np.int16)) + rs.randint(-6, 7, (480, 640, 3)), 0, 255).astype(np.uint8))
    return out


def pipeline_time(n_images, batch, rounds):
    import cls_score_ref as ref
    jp = importlib.import_module("pytorch-human-pose_amd.keypoints.jpeg")
    net = pkg.ClassificationHRNet(32, N)
    net.load_state_dict({k: torch.from_numpy(pkg.synth.synth_param(k, v.shape, 3)) for k, v in net.state_dict().items()})
    model = cls.InferenceClassificationModel(net, {i: f"class-{i}" for i in range(N)}, input_size=256, device=DEV)
    arrays = synthetic_images(n_images)
    jpegs = []
    for i in range(0, n_images, batch):
        jpegs += jp.encode_jpeg_device(arrays[i:i + batch], 90, "420")
    targets = np.random.RandomState(1).randint(0, N, n_images).tolist()
    sets = {"arrays": arrays, "jpeg": jpegs}
    counts, split = {}, {m: {"infer_ms": [], "score_ms": []} for m in sets}

    def run(kind, new):
        t0 = time.perf_counter()
        if new:
            r = cls.evaluate_images(model, sets[kind], targets, max_batch=batch, k=K, confusion=True)
            torch.cuda.synchronize()
            counts[kind, new] = (r["n"], round(r["top-1_error"] * r["n"]), round(r[f"top-{K}_error"] * r["n"]))
            return (time.perf_counter() - t0) * 1e3
        records = model.infer_images(sets[kind], max_batch=batch)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        r = ref.restate(torch.from_numpy(np.stack([rec.logits for rec in records])), torch.tensor(targets), K, confusion=True)
        t2 = time.perf_counter()
        counts[kind, new] = (r["rows"], r["rows"] - r["top1"], r["rows"] - r["topk"])
        split[kind]["infer_ms"].append((t1 - t0) * 1e3), split[kind]["score_ms"].append((t2 - t1) * 1e3)
        return (t2 - t0) * 1e3
    modes = [(kind, new) for kind in sets for new in (True, False)]
    for m in modes:  # warm-up: every shape, every pinned buffer
        run(*m)
    for s in split.values():
        s["infer_ms"].clear(), s["score_ms"].clear()
    times = {m: [] for m in modes}
    for _ in range(rounds):
        for m in modes:  # alternating: the shared host drifts
            times[m].append(run(*m))
    name = lambda kind, new: f"{kind}: " + ("evaluate_images" if new else "infer_images + restatement")  # noqa: E731
    return {"images": n_images, "image_hw": [480, 640], "input_size": 256, "batch": batch, "jpeg_bytes_mean": int(np.mean([len(j) for j in jpegs])),
            "ms_per_pass": {name(*m): spread(times[m]) for m in modes},
            "images_per_s_median": {name(*m): n_images / statistics.median(times[m]) * 1e3 for m in modes},
            "baseline_split_ms": {kind: {k: spread(v) for k, v in s.items()} for kind, s in split.items()},
            "counts_equal": all(counts[kind, True] == counts[kind, False] for kind in sets), "counts": {name(*m): counts[m] for m in modes},
            "read_back_bytes_per_image": {"evaluate_images": 0, "evaluate_images(records=True)": (2 * K + 1) * 4, "infer_images": N * 4}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=512)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--kernels", type=int, nargs=2, metavar=("B", "CONFUSION"), default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cls_eval_time: no GPU: nothing is measured without one")
    if a.kernels:
        kernels_only(*a.kernels)
        return
    out = {"call": [call_time(B, c, a.rounds) for B in (32, 256) for c in (False, True)], "evaluate_images": pipeline_time(a.images, a.batch, a.rounds)}
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
