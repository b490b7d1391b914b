#!/usr/bin/env python3
"""Per-family kernel time of a ClassificationHRNet training step from a rocprofv3 run:

  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python3 tools/cls_train_time.py --steps 3 --warmup 2
  python3 tools/cls_train_families.py OUT [steps_in_the_run = 5]

Reads the newest *kernel_stats.csv under OUT and prints a markdown table: family, launches per step, ms per step, share of kernel time.
"""
import csv
import glob
import os
import sys

FAMILIES = [("tail: pool, linear, cross-entropy (new)", ("avgpool", "linear_", "softmax_xent")),
            ("conv forward / data gradient", ("conv_mfma_kernel",)),
            ("conv weight gradient", ("conv_wgrad_kernel",)),
            ("weight-gradient reduction", ("wgrad_reduce_kernel",)),
            ("BatchNorm forward / backward", ("bn_",)),
            ("weight packing", ("pack_weights",)),
            ("fusion sum", ("upadd",)),
            ("torch elementwise / optimizer / copies", ("at::", "at_cuda", "elementwise", "multi_tensor", "Memcpy", "fill"))]


def main():
    out, steps = sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 5
    hits = sorted(glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True), key=os.path.getmtime)
    if not hits:
        sys.exit(f"no kernel_stats.csv under {out}")
    acc = {f: [0, 0.0] for f, _ in FAMILIES}
    acc["other"] = [0, 0.0]
    others = []
    for r in csv.DictReader(open(hits[-1])):
        fam = next((f for f, keys in FAMILIES if any(k in r["Name"] for k in keys)), "other")
        acc[fam][0] += int(r["Calls"])
        acc[fam][1] += float(r["TotalDurationNs"])
        if fam == "other":
            others.append((float(r["TotalDurationNs"]), r["Name"][:90]))
    total = sum(v[1] for v in acc.values())
    print("| family | launches / step | kernel ms / step | share |\n|---|---|---|---|")
    for f, (calls, ns) in acc.items():
        print(f"| {f} | {calls / steps:.0f} | {ns / steps / 1e6:.3f} | {100 * ns / total:.2f} % |")
    print(f"| all kernels | {sum(v[0] for v in acc.values()) / steps:.0f} | {total / steps / 1e6:.3f} | 100 % |")
    for ns, n in sorted(others, reverse=True)[:8]:
        print(f"other: {ns / steps / 1e6:.3f} ms/step  {n}")


if __name__ == "__main__":
    main()
