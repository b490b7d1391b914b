"""The forward of a bf16 and of an fp16 HigherHRNet-W32 in one process, alternated, on the GPU box:

    python tools/forward_f16_time.py                     bf16 against fp16 (both nets of the library in use)
    python tools/forward_f16_time.py --trace fp16        a run of its own for  rocprofv3 --kernel-trace --stats -- python ... : warm-up,
                                                         then 20 forwards of that one dtype and nothing else
    ... --trace fp16 --single-lane                       the same with hh_set_multi_lane(0): no two kernels overlap, so a kernel's
                                                         duration in the trace is its own

B = 32 at 512 x 512, seeded synthetic weights and images, the input and both outputs resident on the device.  After a warm-up of both
nets: ROUNDS alternations (bf16, fp16, bf16, ...) of FORWARDS forwards each, every block of forwards timed with one pair of device
events on the stream the forwards run on.  Printed: each alternation's ms per forward, the two medians, their ratio, and each type's
own spread (max - min) / median over its alternations -- the yardstick a difference between the types has to beat.

The GPU work runs in a child process under a time limit (the parent never opens the device): a hang ends the child, not the shell."""
import importlib
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, S, K, ROUNDS, FORWARDS, WARMUP = 32, 512, 17, 6, 20, 5
LIMIT_S = 240


def child(trace):
    sys.path.insert(0, REPO)
    import numpy as np
    import torch
    pkg = importlib.import_module("pytorch-human-pose_amd")
    dev = "cuda:0"
    dtypes = [trace] if trace else ["bf16", "fp16"]
    nets, outs = {}, {}
    x = torch.from_numpy(pkg.synth.synth_images(B, S, S, 0)).to(dev)
    for d in dtypes:
        net = pkg.HigherHRNet(K, 32, dtype=d)
        net.load_state_dict({k: torch.from_numpy(pkg.synth.synth_param(k, v.shape, 0)) for k, v in net.state_dict().items()})
        nets[d] = net.to(dev).eval()
        if "--single-lane" in sys.argv:
            net.use_graph = False
            pkg._lib.check(pkg._lib.load().hh_set_multi_lane(net._h, 0))
        outs[d] = (torch.empty((B, 2 * K, S // 4, S // 4), device=dev), torch.empty((B, K, S // 2, S // 2), device=dev))

    def block(d, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.no_grad():
            e0.record()
            for _ in range(n):
                nets[d].forward_raw(x, outs[d])
            e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / n

    for d in dtypes:
        block(d, WARMUP)
    if trace:
        print(f"traced: {FORWARDS} forwards of the {trace} net, {block(trace, FORWARDS):.3f} ms per forward")
        return
    ms = {d: [] for d in dtypes}
    for r in range(ROUNDS):
        for d in dtypes:
            ms[d].append(block(d, FORWARDS))
        print(f"alternation {r}: " + ", ".join(f"{d} {ms[d][-1]:.3f} ms" for d in dtypes))
    med = {d: float(np.median(ms[d])) for d in dtypes}
    spread = {d: (max(ms[d]) - min(ms[d])) / med[d] for d in dtypes}
    for d in dtypes:
        print(f"{d}: median {med[d]:.3f} ms per forward ({B / med[d] * 1e3:.0f} img/s), own spread (max - min) / median {100 * spread[d]:.2f} %")
    print(f"ratio fp16 / bf16: {med['fp16'] / med['bf16']:.4f}  (fp16 is {'slower' if med['fp16'] > med['bf16'] else 'not slower'}; "
          f"difference {100 * (med['fp16'] / med['bf16'] - 1):+.2f} % against bf16's own spread of {100 * spread['bf16']:.2f} %)")
    finite = all(bool(torch.isfinite(t).all()) for d in dtypes for t in outs[d])
    print(f"outputs finite: {finite}; B = {B}, {S} x {S}, {ROUNDS} alternations of {FORWARDS} forwards, warm-up {WARMUP}")


def main():
    if "--child" in sys.argv:
        i = sys.argv.index("--child")
        return child(sys.argv[i + 1] if len(sys.argv) > i + 1 and sys.argv[i + 1] in ("bf16", "fp16") else None)
    trace = sys.argv[sys.argv.index("--trace") + 1] if "--trace" in sys.argv else ""
    if "--trace" in sys.argv:
        return child(trace)  # (under rocprofv3 the program itself is the traced process; its own time limit goes in front of rocprofv3)
    try:
        rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], timeout=LIMIT_S).returncode
    except subprocess.TimeoutExpired:
        print(f"forward_f16_time: the GPU child did not finish within {LIMIT_S} s and was ended")
        rc = 124
    sys.exit(rc)


if __name__ == "__main__":
    main()
