#!/usr/bin/env python3
"""Does a source change leave the device code alone?  Compares the gfx950 assembly of two source trees.

Every translation unit of pytorch-human-pose_amd/csrc (the .hip files and the .cpp files the Makefile compiles with -x hip) is
compiled device-only with the flags the tree's own Makefile gives it (`make -n -B` is asked for the commands, so -ffp-contract=off
of the decode files and anything else per-file is included).  Comment lines, `.file` / `.ident` lines and the `__hip_cuid_*`
symbol (a hash of the source path) are dropped; what is left must be the same text.  Per file: identical / N lines differ, and for
each kernel whose register or scratch figures changed, both sets of figures.

    git worktree add /tmp/parent HEAD~1          (or: git archive HEAD~1 | tar -x -C /tmp/parent)
    python3 tools/isa_diff.py /tmp/parent . [file.hip ...] [-v]       exit code 0 = every translation unit identical

--kernels ARG: for a change that turns kernels into templates over a new leading type argument ARG (e.g. ElemBF16) and adds further
instantiations.  The text of a file then differs by construction, so the comparison is kernel by kernel: every kernel of the first
tree must exist in the second under the same demangled name once "ARG, " is taken out of it, with the same instructions (its own
symbol replaced by a placeholder) and the same register and scratch figures.  Kernels only the second tree has are listed, not judged.
"""
import difflib
import os
import re
import shlex
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

from check_lds_wait_isa import device_asm

FIGURES = (".vgpr_count", ".sgpr_count", ".vgpr_spill_count", ".private_segment_fixed_size")


def units(tree: str):
    """-> (csrc directory, {source file: compiler flags}) from the Makefile's own commands"""
    csrc = os.path.join(os.path.abspath(tree), "pytorch-human-pose_amd", "csrc")
    out = subprocess.check_output(["make", "-n", "-B", "-C", csrc], text=True)
    res = {}
    for ln in out.splitlines():
        tok = shlex.split(ln)
        if "-c" in tok:
            i = tok.index("-c")
            res[tok[i + 1]] = tok[1:i]
    return csrc, res


def normalise(asm: str):
    return [ln for ln in asm.splitlines()
            if not ln.lstrip().startswith((";", ".file", ".ident")) and "__hip_cuid_" not in ln]


def figures(asm: str):
    """-> {kernel: {figure: value}} from the amdhsa.kernels metadata"""
    res, cur = {}, None
    for ln in asm.splitlines():
        if re.match(r"^  - \.", ln):
            cur = {}
        m = re.match(r"^\s+(?:- )?(\.\w+):\s+(\S+)$", ln)
        if cur is not None and m:
            if m.group(1) == ".name":
                res[m.group(2)] = cur
            elif m.group(1) in FIGURES:
                cur[m.group(1)] = m.group(2)
    return res


def kernel_bodies(asm: str, drop: str):
    """-> {demangled kernel name without the `drop` template argument: (instructions with the kernel's symbol replaced, figures)}"""
    figs = figures(asm)
    syms = list(figs)
    names = subprocess.run(["c++filt"], input="\n".join(syms), text=True,
                           capture_output=True, check=True).stdout.splitlines()
    res = {}
    for sym, name in zip(syms, names):
        m = re.search(r"^" + re.escape(sym) + r":.*?\n(.*?)^\.Lfunc_end\d+:", asm, flags=re.M | re.S)
        # (local labels carry the function's index in the file, which the added instantiations shift; so do the comments behind them)
        body = [re.sub(r"\.LBB\d+_", ".LBB_", re.sub(r"\s*;.*$", "", ln).replace(sym, "KERNEL")) for ln in normalise(m.group(1))
                if not ln.lstrip().startswith((".text", ".section"))]  # (a template instantiation gets a comdat section of its own)
        res[re.sub(r"^void ", "", name.replace(drop + ", ", "").replace("<" + drop + ">", ""))] = (body, figs[sym])
    return res


def compare_kernels(job, drop):
    name, (dir_a, flags_a), (dir_b, flags_b) = job
    a = kernel_bodies(device_asm(os.path.join(dir_a, name), flags_a, dir_a), drop)
    b = kernel_bodies(device_asm(os.path.join(dir_b, name), flags_b, dir_b), drop)
    bad = [k for k in a if k not in b or a[k] != b[k]]
    return name, bad, len(a), sorted(set(b) - set(a))


def compare(job):
    name, (dir_a, flags_a), (dir_b, flags_b) = job
    a = device_asm(os.path.join(dir_a, name), flags_a, dir_a)
    b = device_asm(os.path.join(dir_b, name), flags_b, dir_b)
    diff = [ln for ln in difflib.unified_diff(normalise(a), normalise(b), n=0, lineterm="") if ln[:1] in "+-" and ln[:3] not in ("+++", "---")]
    return name, diff, figures(a), figures(b)


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "-v"]
    verbose = "-v" in sys.argv[1:]
    drop = None
    if "--kernels" in args:
        i = args.index("--kernels")
        drop = args[i + 1]
        del args[i:i + 2]
    if len(args) < 2:
        sys.exit(__doc__)
    (dir_a, ua), (dir_b, ub) = units(args[0]), units(args[1])
    names = args[2:] or sorted(set(ua) | set(ub))
    rc = 0
    jobs = []
    for n in names:
        if n not in ua or n not in ub:
            print(f"{n}: only in {args[0] if n in ua else args[1]}")
            rc = 1
        else:
            jobs.append((n, (dir_a, ua[n]), (dir_b, ub[n])))
    if drop:
        with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
            for name, bad, n, new in pool.map(lambda j: compare_kernels(j, drop), jobs):
                print(f"{name}: " + (f"{len(bad)} of {n} kernels differ or are missing" if bad else f"all {n} kernels identical") + f"; {len(new)} new kernels")
                rc |= bool(bad)
                for k in bad + (new if verbose else []):
                    print("    " + k)
        sys.exit(rc)
    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
        for name, diff, fa, fb in pool.map(compare, jobs):
            print(f"{name}: " + (f"{len(diff)} lines differ" if diff else "identical") + f"  ({len(fb)} kernels)")
            rc |= bool(diff)
            for k in sorted(set(fa) | set(fb)):
                if fa.get(k) != fb.get(k) or verbose:
                    show = lambda f: " ".join(f"{key[1:]}={f[key]}" for key in FIGURES if key in f) if f is not None else "absent"
                    print(f"    {k}\n        {args[0]}: {show(fa.get(k))}\n        {args[1]}: {show(fb.get(k))}")
            if verbose:
                print("\n".join("    " + ln for ln in diff[:40]))
    sys.exit(rc)
