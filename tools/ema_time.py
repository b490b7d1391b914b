#!/usr/bin/env python3
"""Time the weight EMA on HigherHRNet-W32's parameter set (no forward or backward: random gradients of the parameters' shapes):

  step       optim.Adam.step() alone -- no EMA attached: hh_optim_step, the launch of before this feature (tools/isa_diff.py shows its
             kernels unchanged), so this is also the parent commit's figure
  torch_ema  the same step followed by torch.optim.swa_utils.AveragedModel.update_parameters (get_ema_multi_avg_fn), what a trainer
             did before
  fused      the step with an attached optim.ModelEMA: one launch (plus the one-workgroup counter launch)
  update     optim.ModelEMA.update() alone, the stand-alone launch
  swap       ema.swap() twice (into the averaged weights and back), against
  reload     the two load_state_dict round trips it replaces (keep a copy of the weights, load the averages, load the copy back)

  python3 tools/ema_time.py [--steps 50] [--warmup 10] [--repeats 5] [--decay 0.9998] [--use-buffers] [--only NAME] [--out result.json]

Each variant is timed `repeats` times, the variants alternating inside every repeat, as a host clock around `steps` calls that end in a
device synchronise; the figures are the median and the lowest and highest repeat (the run-to-run spread inside one process).  Per
variant the script also reports whether torch saw a host synchronisation in one call (torch.cuda.set_sync_debug_mode; it sees torch's
own, such as AveragedModel's bool(n_averaged == 0), not a library's).  Kernel time and launch counts: run `--only NAME --steps 5
--warmup 0 --repeats 1` under `rocprofv3 --kernel-trace --stats` in a call of its own and divide by 5.  Needs the GPU; prints one JSON
line.
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time
import warnings

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
pkg = importlib.import_module("pytorch-human-pose_amd")
optim = pkg.optim
DEV = "cuda:0"


def make_net(seed=0):
    net = pkg.HigherHRNet(17, 32)
    net.load_state_dict({k: torch.from_numpy(pkg.synth.synth_param(k, v.shape, seed)) for k, v in net.state_dict().items()})
    net.to(DEV).train()
    g = torch.Generator(device=DEV).manual_seed(1)
    for p in net.parameters():
        p.grad = torch.empty_like(p, memory_format=torch.preserve_format).normal_(generator=g).mul_(1e-3)
    return net


class Shell(torch.nn.Module):
    """The net's parameters and buffers (the same tensor objects) without its engine handle: AveragedModel deep-copies what it is
    given, and what it averages and copies per step is decided by these alone."""

    def __init__(self, net):
        super().__init__()
        self.ps = torch.nn.ParameterList(list(net.parameters()))
        for i, b in enumerate(net.buffers()):
            self.register_buffer(f"b{i}", b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--decay", type=float, default=0.9998)
    ap.add_argument("--use-buffers", action="store_true")
    ap.add_argument("--only", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ema_time.py needs the GPU: there is nothing to time without one")
    from torch.optim.swa_utils import AveragedModel, get_ema_multi_avg_fn

    # one net and optimizer per variant, so that no variant's state or attachment leaks into another
    plain_net = make_net()
    plain_opt = optim.Adam(plain_net.parameters(), lr=1e-3)
    torch_net = make_net()
    torch_opt = optim.Adam(torch_net.parameters(), lr=1e-3)
    shell = Shell(torch_net)
    averaged = AveragedModel(shell, multi_avg_fn=get_ema_multi_avg_fn(a.decay), use_buffers=a.use_buffers)
    fused_net = make_net()
    fused_opt = optim.Adam(fused_net.parameters(), lr=1e-3)
    fused_ema = optim.ModelEMA(fused_net, fused_opt, decay=a.decay, use_buffers=a.use_buffers)
    alone_net = make_net()
    alone_ema = optim.ModelEMA(alone_net, None, decay=a.decay, use_buffers=a.use_buffers)
    alone_ema.update()
    avg_sd = {k: v.clone() for k, v in alone_ema.state_dict()["model"].items()}

    def torch_ema():
        torch_opt.step()
        averaged.update_parameters(shell)

    def swap():
        alone_ema.swap()
        alone_ema.swap()

    def reload():
        backup = {k: v.clone() for k, v in alone_net.state_dict().items()}
        alone_net.load_state_dict(avg_sd)
        alone_net.load_state_dict(backup)

    variants = {"step": plain_opt.step, "torch_ema": torch_ema, "fused": fused_opt.step, "update": alone_ema.update, "swap": swap, "reload": reload}
    if a.only:
        variants = {a.only: variants[a.only]}
    numel = sum(p.numel() for p in plain_net.parameters())
    res = dict(parameters=numel, tensors=len(list(plain_net.parameters())), averaged_tensors=len(fused_ema.averages), steps=a.steps, warmup=a.warmup,
               repeats=a.repeats, decay=a.decay, use_buffers=a.use_buffers, variants={})
    for fn in variants.values():
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in variants}
    for _ in range(a.repeats):
        for name, fn in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / a.steps * 1e6)
    for name, fn in variants.items():
        torch.cuda.synchronize()
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            torch.cuda.set_sync_debug_mode("warn")
            try:
                fn()
            finally:
                torch.cuda.set_sync_debug_mode("default")
        syncs = [str(w.message)[:160] for w in caught if "called a synchronizing" in str(w.message)]  # (not the mode's own notice)
        t = times[name]
        res["variants"][name] = dict(us_median=statistics.median(t), us_min=min(t), us_max=max(t), host_syncs_seen_by_torch=len(syncs),
                                     sync_warnings=syncs)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
