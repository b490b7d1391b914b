"""Compares the gfx950 kernels of two builds of libhhrnet.so by their code-object metadata, without a GPU: for every kernel the
VGPR, AGPR and SGPR counts, the private-segment (scratch) and group-segment (LDS) sizes and the size of its code.  A refactor that
only renames types must leave all of them as they were.

    python tools/code_object_diff.py OLD.so NEW.so [old_name=new_name ...] > table.md

Kernels are matched by demangled-free name: the mangled name with every `old_name` replaced by `new_name` (length prefixes
included, e.g. 11HHImageDesc=13hh_image_desc).  Exit status 1 if any kernel differs or is unmatched."""
import os
import re
import struct
import subprocess
import sys
import tempfile

LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin", "")
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
KEYS = (".vgpr_count", ".agpr_count", ".sgpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size")


def kernels(so: str) -> dict:
    """{kernel name: (vgpr, agpr, sgpr, scratch, lds, code bytes)} over every gfx950 code object bundled into `so`."""
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        subprocess.check_call([LLVM + "llvm-objcopy", "--dump-section", f".hip_fatbin={tmp}/fatbin", so])
        data = open(f"{tmp}/fatbin", "rb").read()
        for at in (m.start() for m in re.finditer(MAGIC, data)):
            (n,), pos = struct.unpack_from("<Q", data, at + 24), at + 32
            for _ in range(n):
                off, size, idlen = struct.unpack_from("<QQQ", data, pos)
                ident, pos = data[pos + 24:pos + 24 + idlen].decode(), pos + 24 + idlen
                if "gfx950" not in ident or size == 0:
                    continue
                with open(f"{tmp}/co", "wb") as f:
                    f.write(data[at + off:at + off + size])
                notes = subprocess.check_output([LLVM + "llvm-readelf", "--notes", f"{tmp}/co"], text=True)
                symbols = subprocess.check_output([LLVM + "llvm-readelf", "--symbols", "--wide", f"{tmp}/co"], text=True)
                sizes = {m.group(2): int(m.group(1)) for m in re.finditer(r"^\s*\d+:\s+[0-9a-f]+\s+(\d+)\s+FUNC\s+\S+\s+\S+\s+\S+\s+(\S+)$", symbols, flags=re.M)}
                for block in re.split(r"^  - ", notes, flags=re.M)[1:]:
                    top = dict(re.findall(r"^    (\.\w+):\s+(\S+)$", block, flags=re.M))
                    if ".symbol" in top:
                        name = top[".name"].strip("'")
                        out[name] = tuple(int(top.get(k, 0)) for k in KEYS) + (sizes.get(name, -1),)
    return out


def main(old_so: str, new_so: str, *renames: str) -> int:
    old, new = kernels(old_so), kernels(new_so)
    mapped = {}
    for name, meta in old.items():
        for r in renames:
            name = name.replace(*r.split("="))
        mapped[name] = meta
    bad = 0
    print("| kernel | vgpr | agpr | sgpr | scratch | lds | code bytes | against the parent |")
    print("|---|---|---|---|---|---|---|---|")
    for name in sorted(set(mapped) | set(new)):
        a, b = mapped.get(name), new.get(name)
        if a == b:
            verdict = "identical"
        elif a is None or b is None:
            verdict = "only in the " + ("parent" if b is None else "new build")
        else:
            verdict = "; ".join(f"{k.strip('.') if k else 'code bytes'}: {x} -> {y}" for k, x, y in zip(KEYS + ("",), a, b) if x != y)
        bad += verdict != "identical"
        print("| `" + name + "` | " + " | ".join(map(str, b or a)) + " | " + verdict + " |")
    print(f"\n{len(new)} kernels, {bad} not identical")
    return int(bad != 0)


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:]))
