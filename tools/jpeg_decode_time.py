"""Time the device JPEG decoder against the route the reference takes to the same pixels: Pillow's decoder on the host
(`np.array(Image.open(...).convert("RGB"))`) plus the upload of the raw pixels.  32 COCO-sized streams (480 x 640, the synthetic scene,
4:2:0, quality 90, written by Pillow), once with one restart interval per MCU row and once without restarts (decoded through an index).
Both routes in the same process on the same GPU, alternated round by round, after warm-up; medians with the spread (min..max) of the
rounds.  Writes its tables into profiles/jpeg_decode.md between the two `jpeg_decode_time` marker lines, or into --out as a whole file.

    python tools/jpeg_decode_time.py [--rounds 9] [--out FILE]
    python tools/jpeg_decode_time.py --kernels-only 20     # only the decode call, for a kernel trace around it
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
H, W, N = 480, 640, 32


def streams(restart_rows: bool) -> list:
    from PIL import Image
    from jpeg_time import scene
    out = []
    for j in range(N):
        buf = io.BytesIO()
        Image.fromarray(scene(H, W, j)).save(buf, "JPEG", quality=90, subsampling=2, **(dict(restart_marker_rows=1) if restart_rows else {}))
        out.append(buf.getvalue())
    return out


def kernel_ms(J, items: list, rounds: int, dev) -> list:
    """hh_jpeg_decode_u8_batch alone (the clearing of the statuses and the three launches), buffers staged once, by device events"""
    at = (J.DEC_DESC.itemsize * len(items) + 15) // 16 * 16
    places = []
    for it in items:
        places.append(at)
        at += it.staged_bytes()
    stage = np.zeros(at, np.uint8)
    descs = stage[:J.DEC_DESC.itemsize * len(items)].view(J.DEC_DESC)
    out = torch.empty(len(items) * H * W * 3 + 64, dtype=torch.uint8, device=dev)
    ws = np.cumsum([0] + [it.ws_bytes for it in items])
    work = torch.empty(int(ws[-1]), dtype=torch.uint8, device=dev)
    status = torch.zeros(len(items), dtype=torch.int32, device=dev)
    buf = torch.empty(at, dtype=torch.uint8, device=dev)
    base = min(buf.data_ptr(), out.data_ptr())
    for j, it in enumerate(items):
        s_at, t_at = it.stage(stage, places[j])
        descs[j] = (buf.data_ptr() - base + s_at, buf.data_ptr() - base + t_at, it.tables_bytes, out.data_ptr() - base + j * H * W * 3, int(ws[j]), 3 * W,
                    it.data.size, len(it.segments), 0, 0)
    buf.copy_(torch.from_numpy(stage))
    infos = np.concatenate([it.info for it in items])
    times = []
    for r in range(rounds + 3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        J.launch_decode(dev, base, buf.data_ptr(), descs, infos, work, status.data_ptr())
        b.record()
        b.synchronize()
        if r >= 3:
            times.append(a.elapsed_time(b))
    assert not status.any()
    return times


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernels-only", type=int, default=0)
    args = ap.parse_args()
    from PIL import Image
    pkg = importlib.import_module(PKG)
    J = importlib.import_module(PKG + ".keypoints.jpeg")
    ti_mod = pkg.keypoints.train_input
    dev = torch.device("cuda:0")
    sets = {"restart rows": streams(True), "index, one MCU row": streams(False)}
    items = {k: [J.JpegImage(s) for s in v] for k, v in sets.items()}
    for mps in (8, 2):  # the same restart-less streams through finer indexes: more lanes, shorter walks, 32 more table bytes per segment
        items[f"index, {mps} MCUs"] = [J.JpegImage(s, J.build_jpeg_index(s, mps)) for s in sets["index, one MCU row"]]
    if args.kernels_only:
        for k, v in items.items():
            print(k, "3 launches, ms:", statistics.median(kernel_ms(J, v, args.kernels_only, dev)))
        return

    def fmt(ts):
        return f"{statistics.median(ts):.3f} ({min(ts):.3f}..{max(ts):.3f})"

    def pillow(s):
        return np.array(Image.open(io.BytesIO(s)).convert("RGB"))

    def host_route(batch):
        out = [torch.from_numpy(pillow(s)).to(dev, non_blocking=True) for s in batch]
        torch.cuda.synchronize()
        return out

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

    lines = [f"Measured by tools/jpeg_decode_time.py on {torch.cuda.get_device_name(0)}: {N} streams of {H}x{W}, the synthetic scene, 4:2:0, quality 90, "
             f"written by Pillow; {args.rounds} rounds after warm-up, routes alternated in one process; milliseconds, median (min..max).", ""]
    lines += ["| streams | mean bytes | segments per image | hh_jpeg_decode_u8_batch (3 launches) | decode_jpeg_device from bytes, wall | from prepared JpegImage, wall "
              "| Pillow + upload, wall |", "|---|---|---|---|---|---|---|"]
    for k in items:
        kern = kernel_ms(J, items[k], args.rounds, dev)
        if k in sets:
            wall = alternate({"bytes": lambda: J.decode_jpeg_device(sets[k], device=dev), "items": lambda: J.decode_jpeg_device(items[k], device=dev),
                              "host": lambda: host_route(sets[k])})
            lines.append(f"| {k} | {sum(map(len, sets[k])) // N} | {len(items[k][0].segments)} | {fmt(kern)} | {fmt(wall['bytes'])} | {fmt(wall['items'])} | {fmt(wall['host'])} |")
        else:
            wall = alternate({"items": lambda: J.decode_jpeg_device(items[k], device=dev)})
            lines.append(f"| {k} | (the same streams) | {len(items[k][0].segments)} | {fmt(kern)} | - | {fmt(wall['items'])} | - |")

    ti = ti_mod.TrainInput(512, [1 / 4, 1 / 2], device="cuda:0")
    rng = np.random.RandomState(0)
    joints = [np.concatenate([rng.uniform(0, [W, H], (3, 17, 2)), rng.randint(0, 3, (3, 17, 1))], -1) for _ in range(N)]
    mask = np.zeros((H, W), bool)
    params = [ti_mod.AugParams(H / 200, 10.0 * (i % 5) - 20, (W / 2, H / 2), bool(i % 2)) for i in range(N)]
    lines += ["", f"`TrainInput.build` of {N} samples (out_size 512, two stages, dense all-clear crowd masks); the array route includes the Pillow decode the "
              "parent commit needs:", "", "| streams | JpegImage samples, wall | of which JpegImage() on the host | arrays (Pillow decode + build), wall | "
              "bytes staged, JpegImage | bytes staged, arrays |", "|---|---|---|---|---|---|"]
    for k in sets:
        prepared = items[k]
        staged = {}

        def jpeg_build(fresh=False):
            imgs = [J.JpegImage(s) for s in sets[k]] if fresh else prepared
            ti.build([(im, mask, j) for im, j in zip(imgs, joints)], params)
            staged["jpeg"] = ti.last_staged_bytes

        def array_build():
            ti.build([(pillow(s), mask, j) for s, j in zip(sets[k], joints)], params)
            staged["array"] = ti.last_staged_bytes

        wall = alternate({"jpeg": jpeg_build, "array": array_build})
        prep = []
        for _ in range(args.rounds):
            t0 = time.perf_counter()
            [J.JpegImage(s) for s in sets[k]]
            prep.append((time.perf_counter() - t0) * 1e3)
        ti.jpeg_status()
        lines.append(f"| {k} | {fmt(wall['jpeg'])} | {fmt(prep)} (not included: built once per file) | {fmt(wall['array'])} | {staged['jpeg']} | {staged['array']} |")

    idx = []
    for _ in range(args.rounds):
        t0 = time.perf_counter()
        for s in sets["index, one MCU row"]:
            J.build_jpeg_index(s)
        idx.append((time.perf_counter() - t0) * 1e3 / N)
    dec = []
    for _ in range(args.rounds):
        t0 = time.perf_counter()
        for s in sets["index, one MCU row"]:
            pillow(s)
        dec.append((time.perf_counter() - t0) * 1e3 / N)
    lines += ["", f"One-off host cost per image: `build_jpeg_index` {fmt(idx)} ms; for comparison Pillow's whole decode of the same stream {fmt(dec)} ms."]
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out is not None:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
        return
    path = os.path.join(REPO, "profiles", "jpeg_decode.md")
    begin, end = "<!-- jpeg_decode_time:begin -->\n", "<!-- jpeg_decode_time:end -->\n"
    with open(path) as f:
        doc = f.read()
    head, _, rest = doc.partition(begin)
    _, _, tail = rest.partition(end)
    with open(path, "w") as f:
        f.write(head + begin + text + end + tail)


if __name__ == "__main__":
    main()
