"""ctypes binding of csrc/libhhrnet.so (the C-ABI declared in include/hhrnet.h).

There is no CPU fallback: if the HIP library cannot be loaded every product entry point
raises.  `build()` compiles it in-tree with hipcc for gfx950 (works without a GPU).
"""
from __future__ import annotations

import ctypes as C
import functools
import os
import re
import subprocess

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
SO = os.environ.get("HH_LIB") or os.path.join(CSRC, "libhhrnet.so")  # HH_LIB: A/B-test another build of the same ABI
HEADER = os.path.join(os.path.dirname(_HERE), "include", "hhrnet.h")
_lib = None


class HHError(RuntimeError):
    pass


_SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "long long": C.c_int64, "float": C.c_float, "double": C.c_double}


def _kind(decl: str, proto: str, is_return: bool = False):
    """ctypes type of one parameter declaration (`const float mean[3]`, `int64_t P`) or of a return type."""
    decl = " ".join(decl.replace("*", " * ").split())
    if re.fullmatch(r"const char \*( \w+)?", decl):
        return C.c_char_p
    if is_return:
        if decl == "void":
            return None
        if decl in ("hh_net *", "hh_decoder *"):  # a handle
            return C.c_void_p
        base = decl
    else:
        if re.fullmatch(r"(const )?[\w ]+( \*( const)?)+ \w+", decl) or re.fullmatch(r"(const )?[\w ]+ \w+\[\d+\]", decl):
            return C.c_void_p  # accepts ints, None, ctypes arrays, byref() and data_as(POINTER(...))
        base = re.sub(r"^const ", "", decl).rpartition(" ")[0]  # drop the parameter's name
    if base not in _SCALARS:
        raise HHError(f"{HEADER}: cannot derive a ctypes type for `{decl}` in `{proto}`")
    return _SCALARS[base]


def parse_header(text: str) -> tuple[dict, dict]:
    """include/hhrnet.h -> ({entry point: (restype, [argtypes])}, {HH_* macro with an integer value: value}).  Every statement that
    is not a typedef or an enum must be a prototype `ret hh_name(args);` whose types are known: anything else raises, nothing is
    guessed (a wrong argument kind would corrupt a call silently)."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    consts = {k: int(v) for k, v in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(HH_\w+)[ \t]+(\d+)[ \t]*$", text, flags=re.M)}
    text = re.sub(r"^[ \t]*#[^\n]*$", " ", text, flags=re.M)  # preprocessor lines
    text = re.sub(r"\{[^{}]*\}", " ", text)                  # struct and enum bodies
    text = re.sub(r'extern\s+"C"\s*\{|\}', " ", text)        # the extern "C" bracket
    sigs = {}
    for stmt in text.split(";"):
        proto = " ".join(stmt.split())
        if not proto or re.match(r"(typedef|enum)\b", proto):
            continue
        m = re.fullmatch(r"(.*?)\b(hh_\w+) ?\(([^()]*)\)", proto)
        if m is None or m.group(2) in sigs:
            raise HHError(f"{HEADER}: not a prototype this binding understands (or a repeated one): `{proto}`")
        ret, name, params = m.groups()
        params = [] if params.strip() == "void" else params.split(",")
        sigs[name] = (_kind(ret, proto, is_return=True), [_kind(p, proto) for p in params])
    return sigs, consts


@functools.cache
def _header() -> tuple[dict, dict]:
    with open(HEADER) as f:
        return parse_header(f.read())


# the act_dtype of the *_dt training entry points
ACT_BF16, ACT_F16 = _header()[1]["HH_ACT_BF16"], _header()[1]["HH_ACT_F16"]


def build(force: bool = False, jobs: int = 8) -> str:
    args = ["make", "-C", CSRC, f"-j{jobs}"]
    if force:
        args.append("-B")
    subprocess.check_call(args, stdout=subprocess.DEVNULL)
    return SO


def signatures() -> dict:
    """{entry point: (restype, [argtypes])} for every prototype of include/hhrnet.h (parsed once)."""
    return _header()[0]


def _sig(lib) -> None:
    for name, (res, args) in signatures().items():
        if name.startswith("hh_debug_") and not hasattr(lib, name):
            continue  # (test / probe hooks only: an older build of the same ABI behind HH_LIB may lack one)
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args


def exported_symbols() -> list[str]:
    """Entry points declared in include/hhrnet.h."""
    return sorted(signatures())


def load() -> C.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(SO):
            # Normally __graft_entry__.build() has produced the library.  As a convenience a missing one is built here, under an
            # exclusive file lock so that the ranks of a torchrun launch do not compile into the same tree at once (the first
            # holder builds, the others find the finished file), and never once this process has touched the GPU (a compiler
            # child process next to a live HIP context is what the GPU boxes forbid under rocprofv3).
            import fcntl
            if torch.cuda.is_initialized():
                raise HHError(f"{SO} is missing; run __graft_entry__.build() before any GPU work")
            with open(os.path.join(CSRC, ".build.lock"), "w") as lock:
                fcntl.flock(lock, fcntl.LOCK_EX)
                try:
                    if not os.path.exists(SO):
                        build()
                except Exception as e:  # noqa: BLE001
                    raise HHError(f"{SO} is missing and could not be built ({e}); run __graft_entry__.build()") from e
                finally:
                    fcntl.flock(lock, fcntl.LOCK_UN)
        lib = C.CDLL(SO)
        _sig(lib)
        if lib.hh_abi_version() != _header()[1]["HH_ABI_VERSION"]:
            raise HHError("libhhrnet.so ABI version mismatch")
        _lib = lib
    return _lib


def check(rc: int) -> None:
    if rc != 0:
        raise HHError(load().hh_last_error().decode())


def launch(dev, fn, *args) -> None:
    """The one way Python enqueues device work: entry point `fn` with `args` and, last, the current stream of `dev`, with `dev`
    made current (the library launches on the current device).  The stream is read inside the guard at call time, so inside a
    `torch.cuda.stream(...)` block it is the block's stream."""
    with torch.cuda.device(dev):
        check(fn(*args, torch.cuda.current_stream(dev).cuda_stream))


def ptr(t):
    """The device address of an optional tensor: None (NULL) for None."""
    return t.data_ptr() if t is not None else None
