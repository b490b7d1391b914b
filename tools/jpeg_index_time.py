"""Time the JPEG index built on the device (hh_jpeg_index_device_batch) against the routes of the parent commit: an index built on the
host inside the call (from bytes), and an index prepared beforehand.  The 32 restart-less 480 x 640 streams of tools/jpeg_decode_time.py
(the synthetic scene, 4:2:0, quality 90, written by Pillow); every route in one process on one GPU, alternated round by round after
warm-up; medians with the spread (min..max) of the rounds.  Also what synchronisation costs (the counts of the host twin, which runs
the kernel's procedure), and InferenceKeypointsModel.infer_images over 64 files fed bytes, Pillow arrays, or host-indexed JpegImages.
Writes its tables into profiles/jpeg_index.md between the two `jpeg_index_time` marker lines, or into --out as a whole file.

    python tools/jpeg_index_time.py [--rounds 9] [--out FILE]
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

from jpeg_decode_time import H, N, W, streams  # noqa: E402


def call_ms(J, items: list, rounds: int, dev, mps, decode: bool, index: bool = True, subseq=None) -> list:
    """The index call alone, or the index call and the decode call behind it, buffers staged once, by device events."""
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
    status = torch.zeros(2 * len(items), dtype=torch.int32, device=dev)
    buf = torch.empty(at, dtype=torch.uint8, device=dev)
    base = min(buf.data_ptr(), out.data_ptr())
    for j, it in enumerate(items):
        s_at, t_at = it.stage(stage, places[j])
        descs[j] = (buf.data_ptr() - base + s_at, buf.data_ptr() - base + t_at, it.tables_bytes, out.data_ptr() - base + j * H * W * 3, int(ws[j]), 3 * W,
                    it.data.size, it.nseg, 0, 0)
    buf.copy_(torch.from_numpy(stage))
    infos = np.concatenate([it.info for it in items])
    times = []
    for r in range(rounds + 3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        if index:
            J.launch_index(dev, base, buf.data_ptr(), descs, infos, mps, subseq, status.data_ptr() + 4 * len(items))
        if decode:
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
    args = ap.parse_args()
    from PIL import Image
    pkg = importlib.import_module(PKG)
    J = importlib.import_module(PKG + ".keypoints.jpeg")
    dev = torch.device("cuda:0")
    data = streams(False)
    mcols = J.jpeg_info(data[0]).mcu_cols
    lanes, subseq, _, default_mps = J.index_config()

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

    sizes = [("2", 2), ("8", 8), ("one MCU row", mcols)]
    lines = [f"Measured by tools/jpeg_index_time.py on {torch.cuda.get_device_name(0)}: {N} streams of {H}x{W}, the synthetic scene, 4:2:0, quality 90, "
             f"no restart markers, written by Pillow (mean {sum(map(len, data)) // N} bytes); {args.rounds} rounds after warm-up, routes alternated in one "
             f"process; milliseconds, median (min..max).  The index kernel: {lanes} lanes per workgroup, subsequences of {subseq} bytes.", ""]
    lines += ["| MCUs per segment | entries per image | hh_jpeg_index_device_batch alone | index + decode launches | decode launches alone, same entries from the host "
              "(the parent's call) |", "|---|---|---|---|---|"]
    dev_items, host_items = {}, {}
    for label, mps in sizes:
        dev_items[label] = [J.JpegImage(s, "device", mps) for s in data]
        host_items[label] = [J.JpegImage(s, J.build_jpeg_index(s, mps)) for s in data]
        lines.append(f"| {label} | {dev_items[label][0].nseg} | {fmt(call_ms(J, dev_items[label], args.rounds, dev, mps, False))} | "
                     f"{fmt(call_ms(J, dev_items[label], args.rounds, dev, mps, True))} | {fmt(call_ms(J, host_items[label], args.rounds, dev, mps, True, False))} |")

    lines += ["", f"The index call alone at {default_mps} MCUs per segment against the length of a subsequence (the default is {subseq}), with the passes "
              "the host twin counts for it:", "", "| subseq_bytes | subsequences per image (mean) | rounds (mean) | passes, mean | passes, worst image | hh_jpeg_index_device_batch alone |",
              "|---|---|---|---|---|---|"]
    for sub in (16, 32, 64, 128, 256, 512):
        rows = [J.index_sync_host(s, default_mps, sub, lanes)[2] for s in data]
        lines.append(f"| {sub} | {statistics.mean(r['subsequences'] for r in rows):.0f} | {statistics.mean(r['rounds'] for r in rows):.2f} | "
                     f"{statistics.mean(r['iterations'] for r in rows):.2f} | {max(r['iterations'] for r in rows)} | "
                     f"{fmt(call_ms(J, dev_items[sizes[0][0]], args.rounds, dev, default_mps, False, subseq=sub))} |")

    uploaded = {}

    def route(key, fn):
        def run():
            fn()
            uploaded[key] = J.decode_jpeg_device.last_h2d_bytes
        return run

    routes = {"parent: from bytes, host index inside the call (one MCU row)": route("pb", lambda: J.decode_jpeg_device(data, device=dev))}
    for label, mps in sizes:
        routes[f"from bytes, index=\"device\", {label}"] = route("b" + label, lambda mps=mps: J.decode_jpeg_device(data, "device", device=dev, mcus_per_segment=mps))
    for label, _ in sizes:
        routes[f"parent: from prepared JpegImage, host index, {label}"] = route("ph" + label, lambda label=label: J.decode_jpeg_device(host_items[label], device=dev))
        routes[f"from prepared JpegImage, index=\"device\", {label}"] = route("pd" + label, lambda label=label: J.decode_jpeg_device(dev_items[label], device=dev))
    wall = alternate(routes)
    lines += ["", f"`decode_jpeg_device` of the {N} streams, wall clock (staging, one pinned copy, the calls, the read of the statuses):", "",
              "| route | wall | bytes uploaded |", "|---|---|---|"]
    keys = ["pb"] + ["b" + label for label, _ in sizes] + [k + label for label, _ in sizes for k in ("ph", "pd")]  # (in the order the routes were added)
    for name, key in zip(routes, keys):
        lines.append(f"| {name} | {fmt(wall[name])} | {uploaded[key]} |")

    # what synchronisation costs: the host twin runs the kernel's procedure and counts
    def sync_counts(batch, mps):
        rows = [J.index_sync_host(s, mps, subseq, lanes)[2] for s in batch]
        its = [r["iterations"] for r in rows]
        return (f"{statistics.mean(its):.2f}", max(r["iterations_worst"] for r in rows), f"{statistics.mean(r['rounds'] for r in rows):.2f}",
                f"{sum(r['blocks_decoded'] for r in rows) / sum(r['blocks_true'] for r in rows):.3f}",
                f"{statistics.mean(r['subsequences'] for r in rows):.0f}")

    rng = np.random.default_rng(11)
    noise = rng.integers(0, 256, (120, 200, 3), dtype=np.uint8)
    stress = {}
    for q in (1, 100):
        f = io.BytesIO()
        Image.fromarray(noise, "RGB").save(f, "JPEG", quality=q, subsampling=0)
        stress[f"120x200 noise, 4:4:4, quality {q}"] = [f.getvalue()]
    lines += ["", f"Synchronisation, from the counts of hh_debug_jpeg_index_sync_host ({lanes} lanes, subsequences of {subseq} bytes, {default_mps} MCUs per segment): "
              "passes that changed a lane, per image; decoded blocks (speculative walks, repeated walks and the last walk) over the blocks of the "
              "true chain (the last walk).", "", "| streams | subsequences (mean) | rounds (mean) | passes, mean | passes, worst round | blocks decoded / blocks of the image |",
              "|---|---|---|---|---|---|"]
    for name, batch in [(f"the {N} timing streams", data)] + list(stress.items()):
        mean, worst, rounds, ratio, nsub = sync_counts(batch, default_mps)
        lines.append(f"| {name} | {nsub} | {rounds} | {mean} | {worst} | {ratio} |")

    # infer_images over 64 files
    net = pkg.HigherHRNet(17, 32)
    net.load_state_dict({k: torch.from_numpy(pkg.synth.synth_param(k, v.shape, 3)) for k, v in net.state_dict().items()})
    model = pkg.InferenceKeypointsModel(net.to(dev).eval(), det_thr=0.05, tag_thr=0.5, use_flip=False, input_size=512, device=dev)
    files = data + data
    h2d = {}

    def pillow(s):
        return np.array(Image.open(io.BytesIO(s)).convert("RGB"))

    def infer(key, make):
        def run():
            model.infer_images([make(s) for s in files], max_batch=32)
            h2d[key] = model.last_h2d_bytes
        return run

    iw = alternate({"bytes": infer("bytes", lambda s: s), "pillow": infer("pillow", pillow), "host": infer("host", lambda s: J.JpegImage(s))})
    lines += ["", f"`InferenceKeypointsModel.infer_images` over {len(files)} files in memory (HigherHRNet-W32, synthetic weights, input size 512, no flip, batches of 32), "
              "the input formed inside the timed loop; img/s from the median wall time:", "", "| input | wall, ms | img/s | bytes uploaded |", "|---|---|---|---|"]
    for key, name in (("bytes", "bytes in, index on the device"), ("pillow", "Pillow decode on the host, arrays in (the reference's route)"),
                      ("host", "JpegImage(bytes) built in the loop: host index, one MCU row")):
        lines.append(f"| {name} | {fmt(iw[key])} | {len(files) / statistics.median(iw[key]) * 1e3:.0f} | {h2d[key]} |")
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out is not None:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
        return
    path = os.path.join(REPO, "profiles", "jpeg_index.md")
    begin, end = "<!-- jpeg_index_time:begin -->\n", "<!-- jpeg_index_time:end -->\n"
    with open(path) as f:
        doc = f.read()
    head, _, rest = doc.partition(begin)
    _, _, tail = rest.partition(end)
    with open(path, "w") as f:
        f.write(head + begin + text + end + tail)


if __name__ == "__main__":
    main()
