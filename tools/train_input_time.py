#!/usr/bin/env python3
"""Time the input of one training step: the host path (numpy target generators + KeypointsModule.batch_to_device of fp32 images,
heatmaps and masks) against the device path (keypoints/train_input.py: one pinned copy of uint8 pixels, masks and descriptors,
then the warp, mask and render launches), at B = 32, 512^2, 10 people per image.

  python3 tools/train_input_time.py [--batch 32] [--size 512] [--people 10] [--iters 20] [--mosaic P] [--out result.json]

Times are host clocks around work that ends in a device synchronise (the whole call, host staging included) and, for the render
kernels and the hipMemsetAsync of the same output buffers (the write-bandwidth floor), HIP events around back-to-back launches,
alternated in the same run.  The host path has no warp at all (the reference does it with cv2 in its dataset workers): its images
are taken as already augmented, which favours it.  Needs the GPU; prints one JSON line.

--mosaic P adds, in the same run and on one set of COCO-sized raw samples (480 x 640, 427 x 640, 640 x 480, 512 x 512): the device
path with mosaic_probability 0 and P (whole call, launches, H2D bytes), the compose launch hh_mosaic_u8_batch alone as HIP-event
time alternated with the hipMemsetAsync of its canvases, and the host numpy path of the same mosaics (tests/cv_resize.py's
mosaic_reference, then the numpy generators on the canvas joints; again without any warp).
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

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))  # cv_resize: the host mosaic
pkg = importlib.import_module("pytorch-human-pose_amd")
ti_mod = importlib.import_module("pytorch-human-pose_amd.keypoints.train_input")
km = importlib.import_module("pytorch-human-pose_amd.keypoints.model")
targets = pkg.keypoints.targets


def median_ms(fn, iters, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def event_ms(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def mosaic_section(a, dev, hip):
    """The rows of --mosaic: see the module text."""
    import random

    import cv_resize as cv
    B, S, K, lib = a.batch, a.size, 17, pkg._lib.load()
    shapes = [(480, 640), (427, 640), (640, 480), (512, 512)]
    pool = [pkg.synth.synth_train_sample(*shapes[b % 4], a.people, 8000 + b) for b in range(B)]
    res = dict(probability=a.mosaic, raw_shapes=shapes)
    for name, prob in (("p0", 0.0), ("p", a.mosaic)):
        ti = ti_mod.TrainInput(S, [1 / 4, 1 / 2], device=dev, mosaic_probability=prob)
        np.random.seed(1)
        random.seed(1)
        entries, params = ti.train.choose(pool, pool)
        ms = median_ms(lambda: ti.build(entries, params), a.iters)
        res[name] = dict(device_path_ms_median_min_max=ms, launches=ti.last_launches, h2d_bytes=int(ti.last_h2d_bytes),
                         mosaics=sum(isinstance(e, ti_mod.Mosaic) for e in entries))
    mosaics = [(e, p) for e, p in zip(entries, params) if isinstance(e, ti_mod.Mosaic)]
    if not mosaics:
        return res
    # ---- the host numpy path of the same mosaics: four resizes and the tiling per sample, then the generators on the canvas joints
    t0 = time.perf_counter()
    canvases = [cv.mosaic_reference(e.tiles, S) for e, _ in mosaics]
    res["host_compose_ms"] = (time.perf_counter() - t0) * 1e3
    gens = [targets.HeatmapGenerator(K, s, 2) for s in ti.hm_sizes]
    t0 = time.perf_counter()
    for (_, _, joints), (_, p) in zip(canvases, mosaics):
        ints = ti.geometry(2 * S, 2 * S, joints, p)[3]
        [gens[i](ints[i]) for i in range(2)]
    res["host_generators_ms"] = (time.perf_counter() - t0) * 1e3
    # ---- the compose launch alone, on a buffer laid out as build() lays it out
    M = len(mosaics)
    flat = [t for e, _ in mosaics for t in e.tiles]
    offs = np.cumsum([0] + [t[0].size for t in flat] + [t[1].size for t in flat])
    desc_off = (int(offs[-1]) + 63) // 64 * 64
    canvas_off = (desc_off + 112 * M + 63) // 64 * 64
    host = np.zeros(canvas_off + M * 16 * S * S, np.uint8)
    descs = host[desc_off:desc_off + 112 * M].view(ti_mod._MOSAIC_DESC)
    for i, (img, mask, _) in enumerate(flat):
        host[offs[i]:offs[i + 1]] = img.reshape(-1)
        host[offs[len(flat) + i]:offs[len(flat) + i + 1]] = (mask * 255).astype(np.uint8).reshape(-1)
    for m in range(M):
        descs[m] = ([(int(offs[4 * m + t]), int(offs[len(flat) + 4 * m + t]), *flat[4 * m + t][0].shape[:2]) for t in range(4)],
                    canvas_off + m * 16 * S * S, canvas_off + m * 16 * S * S + 12 * S * S)
    raw = torch.from_numpy(host).to(dev)
    stream = torch.cuda.current_stream().cuda_stream

    def compose():
        pkg._lib.check(lib.hh_mosaic_u8_batch(raw.data_ptr(), raw.data_ptr() + desc_off, descs.ctypes.data, M, S, stream))

    def memset():
        assert hip.hipMemsetAsync(raw.data_ptr() + canvas_off, 0, M * 16 * S * S, stream) == 0

    compose()
    torch.cuda.synchronize()
    back = raw[canvas_off:canvas_off + 16 * S * S].cpu().numpy()  # the two paths must agree before their times are compared
    assert np.array_equal(back[:12 * S * S].reshape(2 * S, 2 * S, 3), canvases[0][0]), "device canvas differs from tests/cv_resize.py"
    assert np.array_equal(back[12 * S * S:].reshape(2 * S, 2 * S), canvases[0][1].astype(np.uint8) * 255), "device mask canvas differs"
    compose_ms, memset_ms = [], []
    event_ms(compose, 5), event_ms(memset, 5)
    for _ in range(5):
        memset_ms.append(event_ms(memset, a.iters))
        compose_ms.append(event_ms(compose, a.iters))
    torch.cuda.synchronize()
    written, read = M * 16 * S * S, int(offs[-1])  # every canvas byte once; every source byte at least once (upper bound when shrinking by > 2)
    res.update(compose_ms_runs=compose_ms, canvas_memset_ms_runs=memset_ms, compose_bytes_written=written, compose_source_bytes=read,
               compose_gb_per_s=(written + read) / (np.median(compose_ms) * 1e-3) / 1e9, memset_gb_per_s=written / (np.median(memset_ms) * 1e-3) / 1e9)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--people", type=int, default=10)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--mosaic", type=float, default=None, help="also time the device path with this mosaic_probability (and with 0)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("train_input_time.py needs the GPU: there is nothing to time without one")
    dev, B, S, K = "cuda:0", a.batch, a.size, 17
    ti = ti_mod.TrainInput(S, [1 / 4, 1 / 2], device=dev)
    samples = [pkg.synth.synth_train_sample(S, S, a.people, 7000 + b) for b in range(B)]
    np.random.seed(0)
    import random
    random.seed(0)
    params = [ti.train.draw(S, S) for _ in range(B)]

    # ---- host path at the parent's semantics: joints already transformed (float64, tiny), generators in numpy, pageable H2D
    geo = [ti.geometry(S, S, s[2], p) for s, p in zip(samples, params)]
    gens = [targets.HeatmapGenerator(K, s, 2) for s in ti.hm_sizes]
    jgens = [targets.JointsGenerator(s) for s in ti.hm_sizes]
    images_host = torch.from_numpy(pkg.synth.synth_images(B, S, S, 0))
    masks_host = [torch.ones((B, s, s), dtype=torch.float32) for s in ti.hm_sizes]
    module = km.KeypointsModule.__new__(km.KeypointsModule)
    module.model = type("M", (), {"device": dev})()
    loss = importlib.import_module("pytorch-human-pose_amd.keypoints.loss")

    def host_generators():
        joints = [[jgens[i](g[2][i]) for g in geo] for i in range(2)]
        hms = [torch.from_numpy(np.stack([gens[i](j) for j in joints[i]])) for i in range(2)]
        return hms, joints

    def host_upload(hms, joints):
        batch = module.batch_to_device((images_host, hms, masks_host, joints))
        return batch, [loss.upload_joints(joints[i], K, s, s, dev) for i, s in enumerate(ti.hm_sizes)]

    def host_path():
        return host_upload(*host_generators())

    t0 = time.perf_counter()
    for _ in range(3):
        hms, joints = host_generators()
    gen_ms = (time.perf_counter() - t0) / 3 * 1e3
    host_ms = median_ms(host_path, max(3, a.iters // 4), warmup=1)
    upload_ms = median_ms(lambda: host_upload(hms, joints), a.iters)
    packed = [loss.pack_joints(joints[i], K, s, s) for i, s in enumerate(ti.hm_sizes)]
    host_bytes = images_host.numel() * 4 + sum(h.numel() * 4 for h in hms) + sum(m.numel() * 4 for m in masks_host) + sum(p.nbytes + c.nbytes for p, c in packed)

    # ---- device path
    dev_ms = median_ms(lambda: ti.build(samples, params), a.iters)
    images, heatmaps, masks, dj = ti.build(samples, params)
    torch.cuda.synchronize()
    for i in range(2):  # the two paths must agree before their times are compared
        assert torch.equal(heatmaps[i].cpu(), hms[i]), f"stage {i}: device heatmaps differ from the numpy generator"

    # ---- render kernels against hipMemsetAsync of the same buffers, alternated
    lib = pkg._lib.load()
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemsetAsync.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]
    stream = torch.cuda.current_stream().cuda_stream
    tables = ti._tables_dev

    def render():
        for i, s in enumerate(ti.hm_sizes):
            pkg._lib.check(lib.hh_render_heatmaps(dj[i].packed.data_ptr(), dj[i].counts.data_ptr(), B, dj[i].packed.shape[1], K, tables[i].data_ptr(),
                                                  tables[i].shape[0], ti.tables[i][1], heatmaps[i].data_ptr(), s, s, stream))

    def memset():
        for h in heatmaps:
            assert hip.hipMemsetAsync(h.data_ptr(), 0, h.numel() * 4, stream) == 0

    render_ms, memset_ms = [], []
    event_ms(render, 5), event_ms(memset, 5)
    for _ in range(5):
        memset_ms.append(event_ms(memset, a.iters))
        render_ms.append(event_ms(render, a.iters))
    render()
    torch.cuda.synchronize()
    out_bytes = sum(h.numel() * 4 for h in heatmaps)
    res = dict(batch=B, size=S, people=a.people, iters=a.iters,
               host_generators_ms=gen_ms, host_upload_ms_median_min_max=upload_ms, host_path_ms_median_min_max=host_ms, host_h2d_bytes=int(host_bytes),
               device_path_ms_median_min_max=dev_ms, device_launches=ti.last_launches, device_h2d_bytes=int(ti.last_h2d_bytes),
               render_ms_runs=render_ms, memset_ms_runs=memset_ms, render_output_bytes=int(out_bytes),
               render_gb_per_s=out_bytes / (np.median(render_ms) * 1e-3) / 1e9, memset_gb_per_s=out_bytes / (np.median(memset_ms) * 1e-3) / 1e9)
    if a.mosaic is not None:
        res["mosaic"] = mosaic_section(a, dev, hip)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
