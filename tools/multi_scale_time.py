"""Multi-scale + flip test (BASELINE.json configs[3]) per image against batched, on the GPU box:

    python tools/multi_scale_time.py                  the same-run comparison (rates, ratio, spread, workspace, aggregation bytes)
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/multi_scale_time.py --trace
                                                      a run of its own: warm-up, a pause, ONE batched pass (nothing else is timed)
    python tools/multi_scale_time.py --summarise DIR  shares of that batched pass from DIR's kernel trace

HigherHRNet-W48, input_size 640, scales (0.5, 1.0, 2.0), flip, max_batch 32, 64 seeded synthetic uint8 images (480x640 and 640x480
mixed), seeded synthetic weights.  Both paths are timed with a host clock around calls that return finished results
(call_multi_scale / infer_images end in the device->host copy of the decode results), alternately in one process, three rounds
each, after every shape of both paths has run once."""
import csv
import glob
import importlib
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SCALES, INPUT_SIZE, MAX_BATCH, N_IMAGES, ROUNDS, K = (0.5, 1.0, 2.0), 640, 32, 64, 3, 17
HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec (6.29 TB/s measured with a float4 copy)
AGG_KERNEL = "multi_scale_aggregate_kernel"
# every kernel of a chunk that is neither a forward kernel nor the aggregation: preprocessing, the flips, the decode
OTHER = ("preprocess", "flip_images", "flip_merge", "peaks", "topk", "match", "adjust", "refine", "fallback", "nms", "stage_average")


def aggregate_bytes(km, shapes, flip):
    """Algorithmic bytes of the aggregation launches of one pass over `shapes`, from shapes alone: every source map read once (the
    flipped pass's too where the launch merges it: the scales other than 1.0), dst written once.  -> (bytes, launches)"""
    total = launches = 0
    for c in km.plan_multi_scale(shapes, INPUT_SIZE, SCALES, MAX_BATCH):
        n = len(c["images"])
        w1, h1 = c["sizes"][SCALES.index(1.0)]
        cuts = sorted({lo for subs in c["sub_batches"] for lo, _ in subs})
        launches += 2 * len(cuts)
        for div in (4, 2):
            total += 4 * n * K * (h1 // div) * (w1 // div)
            for s, (ws, hs) in zip(SCALES, c["sizes"]):
                total += 4 * n * K * (hs // div) * (ws // div) * (2 if flip and s != 1.0 else 1)
    return total, launches


def union_ns(iv):
    busy, end = 0, None
    for s, e in sorted(iv):
        if end is None or s > end:
            busy += e - s
            end = e
        elif e > end:
            busy += e - end
            end = e
    return busy


def summarise(trace_dir):
    f = max(glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True), key=os.path.getsize)
    rows = sorted(((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(open(f))))
    # the batched pass = everything behind the longest pause between two kernels (--trace sleeps before it)
    cut = max(range(1, len(rows)), key=lambda i: rows[i][0] - max(r[1] for r in rows[max(0, i - 64):i]))
    win = rows[cut:]
    span = max(r[1] for r in win) - win[0][0]
    cls = {"aggregation": [], "other": [], "forward": []}
    for s, e, name in win:
        key = "aggregation" if AGG_KERNEL in name else "other" if any(o in name for o in OTHER) else "forward"
        cls[key].append((s, e))
    print(f"{f}: batched pass = {len(win)} kernels over {span / 1e6:.2f} ms ({span / 1e6 / N_IMAGES:.3f} ms/img)")
    busy = union_ns([iv for v in cls.values() for iv in v])
    for key, iv in cls.items():
        print(f"  {key:12s} {len(iv):6d} launches, some kernel of it running {union_ns(iv) / 1e6:9.3f} ms = {100.0 * union_ns(iv) / span:5.1f} % of the pass"
              f" (summed durations {sum(e - s for s, e in iv) / 1e6:.3f} ms)")
    print(f"  gaps (no kernel running) {(span - busy) / 1e6:.3f} ms = {100.0 * (span - busy) / span:.1f} % of the pass")
    agg = cls["aggregation"]
    if agg:
        print(f"  aggregation launches: {len(agg)}, summed {sum(e - s for s, e in agg) / 1e3:.1f} us (compare with the bytes the timing run prints)")


def main():
    if "--summarise" in sys.argv:
        return summarise(sys.argv[sys.argv.index("--summarise") + 1])
    import torch
    pkg = importlib.import_module("pytorch-human-pose_amd")
    km = importlib.import_module("pytorch-human-pose_amd.keypoints.model")
    net = pkg.HigherHRNet(K, 48)
    net.load_state_dict({k: torch.from_numpy(pkg.synth.synth_param(k, v.shape, 0)) for k, v in net.state_dict().items()})
    model = pkg.InferenceKeypointsModel(net, det_thr=0.05, tag_thr=0.5, use_flip=True, input_size=INPUT_SIZE, device="cuda:0")
    rs = np.random.RandomState(0)
    images = [rs.randint(0, 255, ((480, 640, 3) if i % 2 == 0 else (640, 480, 3))).astype(np.uint8) for i in range(N_IMAGES)]

    def batched():
        t0 = time.perf_counter()
        res = model.infer_images(images, max_batch=MAX_BATCH, scales=SCALES)
        return time.perf_counter() - t0, res

    def per_image():
        t0 = time.perf_counter()
        res = [model.call_multi_scale(im, None, SCALES) for im in images]
        return time.perf_counter() - t0, res

    batched()  # warm-up: every shape of the batched path (the timed passes run the same list) ...
    if "--trace" in sys.argv:
        torch.cuda.synchronize()
        time.sleep(0.5)  # the pause --summarise finds the pass by
        t, _ = batched()
        torch.cuda.synchronize()
        print(f"traced batched pass: {t * 1e3:.1f} ms for {N_IMAGES} images")
        return
    for im in images[:2]:  # ... and both shapes of the per-image path
        model.call_multi_scale(im, None, SCALES)
    tb, tp = [], []
    for _ in range(ROUNDS):
        t, rp = per_image()
        tp.append(t)
        t, rb = batched()
        tb.append(t)
    same = all(np.array_equal(getattr(a, f), getattr(b, f)) for a, b in zip(rb, rp) for f in ("kpts_coords", "kpts_scores", "kpts_tags", "obj_scores"))
    rate_b, rate_p = [N_IMAGES / t for t in tb], [N_IMAGES / t for t in tp]
    med_b, med_p = float(np.median(rate_b)), float(np.median(rate_p))
    print(f"per image (call_multi_scale): {med_p:.1f} img/s median of {[round(r, 1) for r in rate_p]} ({1e3 / med_p:.2f} ms/img), "
          f"spread {max(rate_p) - min(rate_p):.1f}")
    print(f"batched (infer_images, scales={SCALES}, max_batch={MAX_BATCH}): {med_b:.1f} img/s median of {[round(r, 1) for r in rate_b]} "
          f"({1e3 / med_b:.2f} ms/img), spread {max(rate_b) - min(rate_b):.1f}")
    print(f"ratio batched / per image: {med_b / med_p:.2f} (slowest batched round over fastest per-image round: {min(rate_b) / max(rate_p):.2f}); "
          f"results identical in the last round: {same}")
    print(f"net.workspace_bytes(): {net.workspace_bytes()} ({net.workspace_bytes() / 2 ** 30:.2f} GiB); "
          f"torch peak allocated {torch.cuda.max_memory_allocated() / 2 ** 30:.2f} GiB")
    nbytes, launches = aggregate_bytes(km, [im.shape[:2] for im in images], True)
    print(f"aggregation: {launches} launches per pass of {N_IMAGES} images, {nbytes} algorithmic bytes ({nbytes / 1e6:.1f} MB: every source once, dst once); "
          f"at the HBM peak of {HBM_PEAK_GBS:.0f} GB/s that is {nbytes / HBM_PEAK_GBS / 1e3:.1f} us")


if __name__ == "__main__":
    main()
