#!/usr/bin/env python3
"""Time the heatmap panels on the GPU for the inference figure (K = 17 stage-average maps + 17 tag maps, min-max, two grids of two
rows, pad 5, then x 0.6) at a model input of 512 x 512, beside what a host plot has to start with: reading `res.kpts_heatmaps` and
`res.tags_heatmaps` (F.interpolate on the device + 2 K H W fp32 to the host).

  python3 tools/panels_time.py [--iters 30] [--rounds 5] [--size 512] [--no-ref] [--out result.json]

Launch times are HIP-event times over `--iters` back-to-back calls on a table that is already on the device (median, min, max of
`--rounds` rounds).  hh_heatmap_panels_u8 issues the min/max launch and the paint launch from one call, so the two are separated by
timing the call twice: with the min-max flag on every map (both launches) and with the flag cleared (the paint launch alone, which then
skips the division of step 2 and the join of the 32 partial ranges); the min/max launch is reported as the difference.  Call times are
host clocks around one call that ends in a device synchronise, each kind of call timed on its own, `--iters` calls after three
untimed ones (median, min, max): the whole `plot_heatmaps_figure()`, its device part (un-normalise, table upload, the panels call,
the resize) up to a synchronise, `to_host` of the finished figure, and the parent's two properties.  The reference
(tests/panels_ref.py, numpy on the CPU) is timed once on the same maps and compared byte for byte.  Needs the GPU; prints one JSON line."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
pkg = importlib.import_module("pytorch-human-pose_amd")
vz = importlib.import_module("pytorch-human-pose_amd.keypoints.visualization")


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


def call_ms(fn, iters):
    """Host time of one call + synchronise -> (median, min, max) over `iters` calls, after three untimed ones."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out)), float(min(out)), float(max(out))


def direct_call(image, placed, Hc, Wc, flags):
    """A closure that repeats only hh_heatmap_panels_u8 on a table that is already on the device, every map's flags replaced."""
    lib = pkg._lib.load()
    table = vz._panel_table([(k, a, b, flags, oy, ox) for k, a, b, _, oy, ox in placed], lambda t: t.data_ptr())
    t_dev = torch.from_numpy(table.view(np.uint8).copy()).to(image.device)
    lut = torch.from_numpy(vz.jet_lut()).to(image.device)
    canvas = torch.empty((Hc, Wc, 3), dtype=torch.uint8, device=image.device)
    scratch = torch.empty(len(table) * vz.PANEL_PARTS * 2, dtype=torch.float32, device=image.device)
    stream = torch.cuda.current_stream(image.device).cuda_stream

    def fn():
        pkg._lib.check(lib.hh_heatmap_panels_u8(t_dev.data_ptr(), table.ctypes.data, len(table), image.data_ptr(), image.shape[0], image.shape[1],
                                                lut.data_ptr(), canvas.data_ptr(), Hc, Wc, Wc * 3, scratch.data_ptr(), stream))
        return canvas
    return fn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--no-ref", action="store_true", help="skip the CPU reference (its time and the byte comparison)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("panels_time.py needs the GPU: there is nothing to time without one")
    dev = "cuda:0"
    S = a.size
    net = pkg.HigherHRNet(17, 32)
    net.load_state_dict({k: torch.from_numpy(pkg.synth.synth_param(k, v.shape, 3)) for k, v in net.state_dict().items()})
    model = pkg.InferenceKeypointsModel(net.to(dev).eval(), det_thr=0.05, tag_thr=0.5, use_flip=False, input_size=S, device=dev)
    res = model(np.random.RandomState(0).randint(0, 256, (S, S, 3)).astype(np.uint8), None)
    K, (H, W) = 17, tuple(res.model_input_image.shape[-2:])
    hq, hh = (t[0].float().contiguous() for t in res._stage_hms)
    tags = res._tags[0][0].float().contiguous()
    image = vz.unnormalize_device(res.model_input_image)
    grids = [([(vz.AVERAGE, q, h, vz.MINMAX) for q, h in zip(hq, hh)], 2, 5), ([(vz.SINGLE, m, None, vz.MINMAX) for m in tags], 2, 5)]
    placed, Hc, Wc = vz.figure_layout(grids, H, W)
    both, paint = direct_call(image, placed, Hc, Wc, vz.MINMAX), direct_call(image, placed, Hc, Wc, 0)
    canvas = both()

    def resize_only():
        return vz.resize_scaled_device(canvas, 0.6, 0.6)

    def unnormalize_only():
        return vz.unnormalize_device(res.model_input_image)

    def figure_call():
        return res.plot_heatmaps_figure()

    def parent_call():
        return res.kpts_heatmaps, res.tags_heatmaps

    def device_part():
        return vz.figure_device(vz.unnormalize_device(res.model_input_image), grids, 0.6)

    fig_dev = device_part()

    def copy_back():
        return vz.to_host(fig_dev)

    for fn in (both, paint, resize_only, unnormalize_only):
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    t_both, t_paint = event_ms(both, a.iters, a.rounds), event_ms(paint, a.iters, a.rounds)
    t_resize, t_unnorm = event_ms(resize_only, a.iters, a.rounds), event_ms(unnormalize_only, a.iters, a.rounds)
    t_fig, t_dev, t_back, t_parent = (call_ms(fn, a.iters) for fn in (figure_call, device_part, copy_back, parent_call))
    fig = figure_call()
    out = dict(K=K, input=[H, W], canvas=[Hc, Wc], canvas_bytes=Hc * Wc * 3, figure=list(fig.shape), maps=len(placed),
               panels_call_both_launches_ms=t_both, paint_launch_alone_ms=t_paint, minmax_launch_by_difference_ms=t_both[0] - t_paint[0],
               resize_launch_ms=t_resize, unnormalize_launch_ms=t_unnorm, plot_heatmaps_figure_call_ms=t_fig, device_part_call_ms=t_dev, to_host_call_ms=t_back,
               parent_properties_call_ms=t_parent,
               bytes_to_host=dict(figure=int(fig.nbytes), parent_properties=2 * K * H * W * 4))
    if not a.no_ref:
        import panels_ref as pr
        cpu = [t.cpu().numpy() for t in (res.model_input_image, hq, hh, tags)]
        t0 = time.perf_counter()
        want = pr.inference_figure(pr.inverse_transform(cpu[0]), cpu[1], cpu[2], cpu[3], pr.jet_lut())
        out["panels_ref_cpu_ms"] = (time.perf_counter() - t0) * 1e3
        out["figure_equals_panels_ref"] = bool(np.array_equal(fig, want))
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
