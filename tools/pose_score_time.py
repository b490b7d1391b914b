#!/usr/bin/env python3
"""Times the per-image OKS scoring (hh_pose_score_batch; keypoints/pose_score.py) on the GPU and against scoring on the host.

  python3 tools/pose_score_time.py [--images 256] [--size 256] [--batch 32] [--rounds 9] [--out FILE.json]

1. The launch alone: one score_device call (the pinned copy of the target tables, the launch, nothing copied back) on a batch of
   `batch` images of 30 predictions x 8 targets, K = 17, in the DECODE form: device-event time per call over windows of 200 calls, and
   the host's wall time per call (what the enqueueing thread pays).
2. infer_images over a fixed synthetic set (synthetic weights, `images` images of size x size) with annotations of 0 .. 15 objects per
   image, so that every batch has another target count, alternating in every round: score=None; score="oks"; score=None followed by
   calculate_OKS() on every result (the host twin on the copied-back arrays); score=None followed by the numpy restatement of
   tests/pose_score_ref.py on the copied-back arrays.  Wall time per call with a device synchronise at its end; median and the
   min .. max spread over the rounds are printed, nothing is judged.  Besides: the FIRST score="oks" pass of the model (its pinned
   buffers are allocated in it) next to the first score=None pass over the same set, the number of pinned result-buffer sets the model
   holds afterwards, and the host's packing work of one pass (pack_targets and the inverse matrices, what infer_images does per batch
   in front of its launches) timed on its own.
There is no target: the work per image is a few thousand fp64 operations and the launch is latency-bound."""
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
ps = pkg.keypoints.pose_score
DEV = "cuda:0"


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def launch_time(batch, rounds):
    rs = np.random.RandomState(0)
    K, P, T, W = 17, 30, 8, 4
    joints = torch.from_numpy(rs.uniform(0, 500, (batch, P, K, W)).astype(np.float32)).to(DEV)
    scores = torch.from_numpy(rs.uniform(0.1, 0.9, (batch, P)).astype(np.float32)).to(DEV)
    num = torch.full((batch,), P, dtype=torch.int32, device=DEV)
    flags = torch.zeros(batch, dtype=torch.int32, device=DEV)
    xyv = np.concatenate([np.round(rs.uniform(0, 500, (batch * T, K, 2))), rs.randint(1, 3, (batch * T, K, 1))], -1)
    targets = ps.make_targets(xyv, t_off=np.arange(batch + 1) * T, t_area=np.full(batch * T, 9000.0))
    inv = np.tile(np.array([1.7, 0, -3.25, 0, 1.7, 5.5]), (batch, 1))

    def call():
        return ps.score_device(targets, decode=(joints, scores, num, flags), inv_affine=inv)
    for _ in range(20):
        call()
    torch.cuda.synchronize()
    dev_us, host_us, n = [], [], 200
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
    return {"batch": batch, "P": P, "T": T, "K": K, "device_us_per_call": spread(dev_us), "host_enqueue_us_per_call": spread(host_us)}


def pipeline_time(n_images, size, batch, rounds):
    import pose_score_ref as ref
    net = pkg.HigherHRNet(17, 32)
    net.load_state_dict({k: torch.from_numpy(pkg.synth.synth_param(k, v.shape, 3)) for k, v in net.state_dict().items()})
    model = pkg.InferenceKeypointsModel(net.to(DEV).eval(), det_thr=0.05, tag_thr=0.5, use_flip=False, input_size=size, device=DEV)
    rs = np.random.RandomState(5)
    images = [rs.randint(0, 255, (size, size, 3)).astype(np.uint8) for _ in range(n_images)]
    plain = model.infer_images(images, max_batch=batch)
    annots = []
    for res in plain:  # 0 .. 15 people annotated, a few pixels off: the target count differs from batch to batch
        objs = []
        for p in rs.permutation(len(res.kpts_coords))[:rs.randint(0, 16)]:
            xy = np.round(res.kpts_coords[p].astype(np.float64)) + rs.randint(-3, 4, (17, 2))
            objs.append({"keypoints": np.concatenate([xy, np.full((17, 1), 2)], 1).astype(int).reshape(-1).tolist(),
                         "segmentation": [[0, 0, size // 2, 0, size // 2, size // 2, 0, size // 2]]})
        annots.append(objs)

    def run(mode):
        t0 = time.perf_counter()
        res = model.infer_images(images, annots=annots, max_batch=batch, score="oks" if mode == "device" else None)
        if mode == "host_twin":
            vals = [r.calculate_OKS() for r in res]
        elif mode == "numpy":
            vals = []
            for r, a in zip(res, annots):
                tg = ps.pack_targets([a], num_kpts=17)
                vals.append(ref.score_image(r.kpts_coords.astype(np.float64), r.obj_scores.astype(np.float64), tg["t_xyv"], tg["t_area"], tg["t_head"],
                                            ps.OKS_VARIANCES)["value"])
        else:
            vals = [r.oks for r in res]
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, vals
    modes = ("none", "device", "host_twin", "numpy")
    first = {"none": run("none")[0], "device": run("device")[0]}  # `plain` above warmed the kernels up; no score= pass has run yet
    for m in modes:
        run(m)
    results_module = importlib.import_module(pkg.__name__ + ".keypoints.results")
    geo = model._geometry(images[0])
    pack_ms = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        for lo in range(0, n_images, batch):
            ps.pack_targets(annots[lo:lo + batch], "oks", num_kpts=17)
            for _i in range(lo, min(lo + batch, n_images)):
                results_module.inverse_affine(geo[1], geo[2], geo[0])
        pack_ms.append((time.perf_counter() - t0) * 1e3)
    times = {m: [] for m in modes}
    values = {}
    for _ in range(rounds):
        for m in modes:  # alternating: the shared host drifts
            ms, values[m] = run(m)
            times[m].append(ms)
    agree = max(abs(a - b) for a, b in zip(values["device"], values["host_twin"]))
    per_batch = [int(sum(len(a) for a in annots[lo:lo + batch])) for lo in range(0, n_images, batch)]
    return {"images": n_images, "size": size, "batch": batch, "people": int(sum(len(r.kpts_coords) for r in plain)), "targets": int(sum(len(a) for a in annots)),
            "targets_per_batch": per_batch, "first_pass_ms": first, "pinned_result_sets": len(model._out_ring),
            "host_packing_ms_per_pass": spread(pack_ms), "ms_per_call": {m: spread(times[m]) for m in modes}, "largest_device_minus_host_twin": agree}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pose_score_time: no GPU: nothing is measured without one")
    out = {"config": ps.config(), "launch": launch_time(a.batch, a.rounds), "infer_images": pipeline_time(a.images, a.size, a.batch, a.rounds)}
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
