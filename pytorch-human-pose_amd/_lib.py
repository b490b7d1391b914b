"""ctypes binding of csrc/libhhrnet.so (the C-ABI declared in include/hhrnet.h): signatures, constants and the layout of every
descriptor struct are read from that header, which is their only definition.

There is no CPU fallback: if the HIP library cannot be loaded every product entry point
raises.  `build()` compiles it in-tree with hipcc for gfx950 (works without a GPU).
"""
from __future__ import annotations

import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
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


# what a struct field may be made of; a pointer of any type is an address (marked, so that struct_ctype can make it a c_void_p)
_FIELDS = {"int": "<i4", "int32_t": "<i4", "uint32_t": "<u4", "int64_t": "<i8", "long long": "<i8", "float": "<f4", "double": "<f8",
           "uint8_t": "u1", "int16_t": "<i2", "uint16_t": "<u2"}
_POINTER = np.dtype("<u8", metadata={"pointer": True})


def _struct(name: str, body: str, consts: dict, structs: dict) -> np.dtype:
    """The aligned numpy dtype of one `typedef struct hh_x { body } hh_x;`: scalars, pointers (`<u8`), arrays bounded by numbers or
    HH_* macros, earlier hh_* structs."""
    fields = []
    for decl in filter(None, (" ".join(d.replace("*", " * ").split()) for d in body.split(";"))):
        one = r"(?:\* (?:const )?)*\w+(?:\[\w+\])*"  # a declarator: `x`, `* x`, `* const * x`, `x[6]`, `x[HH_N][6]`
        m = re.fullmatch(rf"(?:const )?([\w ]+?) ({one}(?: ?, ?{one})*)", decl)
        base = structs.get(m.group(1)) or _FIELDS.get(m.group(1)) if m else None
        if m is None or base is None and not all("*" in item for item in m.group(2).split(",")):
            raise HHError(f"{HEADER}: cannot derive a field type for `{decl}` in struct {name}")
        for item in m.group(2).split(","):
            field, *dims = re.findall(r"\w+", item.replace("const ", ""))
            shape = tuple(int(d) if d.isdigit() else consts.get(d, -1) for d in dims)
            if min(shape, default=1) < 1:
                raise HHError(f"{HEADER}: array bound of `{field}` in struct {name} is neither a number nor a parsed HH_* macro")
            fields.append((field, _POINTER if "*" in item else base, shape))
    if len({f[0] for f in fields}) != len(fields) or not fields:
        raise HHError(f"{HEADER}: struct {name} is empty or repeats a field name")
    return np.dtype(fields, align=True)


def _parse(text: str) -> tuple[dict, dict, dict]:
    """include/hhrnet.h -> (signatures, constants, struct dtypes); see parse_header and parse_structs."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    consts = {k: int(v) for k, v in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(HH_\w+)[ \t]+(\d+)[ \t]*$", text, flags=re.M)}
    text = re.sub(r"^[ \t]*#[^\n]*$", " ", text, flags=re.M)  # preprocessor lines
    for body in re.findall(r"\benum\s*\{([^{}]*)\}\s*;", text):
        consts.update((k, int(v)) for k, v in re.findall(r"(HH_\w+)\s*=\s*(\d+)\s*(?:,|$)", body))
    text = re.sub(r"\benum\s*\{[^{}]*\}", "enum", text)
    structs = {}

    def struct(m):
        name, body, alias = m.groups()
        if alias != name or "{" in body or name in structs:
            raise HHError(f"{HEADER}: struct {name} nests a struct or union, is not closed by `}} {name};`, or is repeated")
        structs[name] = _struct(name, body, consts, structs)
        return " "
    text = re.sub(r"\btypedef\s+struct\s+(hh_\w+)\s*\{(.*?)\}\s*(\w*)\s*;", struct, text, flags=re.S)
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
    return sigs, consts, structs


def parse_header(text: str) -> tuple[dict, dict]:
    """include/hhrnet.h -> ({entry point: (restype, [argtypes])}, {HH_* macro or enumerator with an integer value: value}).  Every
    statement that is not a typedef or an enum must be a prototype `ret hh_name(args);` whose types are known, and every field of
    every struct body must be understood (parse_structs): anything else raises, nothing is guessed (a wrong argument kind or field
    offset would corrupt a call silently)."""
    return _parse(text)[:2]


def parse_structs(text: str) -> dict:
    """include/hhrnet.h -> {hh_* struct: its numpy dtype, laid out as the C compiler lays it out (align=True)}."""
    return _parse(text)[2]


@functools.cache
def _header() -> tuple[dict, dict, dict]:
    with open(HEADER) as f:
        return _parse(f.read())


def const(name: str) -> int:
    """The value of the macro or enumerator HH_<name> of include/hhrnet.h."""
    return _header()[1]["HH_" + name]


def struct_dtype(name: str) -> np.dtype:
    """The one definition of a descriptor table's row in Python: the dtype derived from the struct's body in include/hhrnet.h."""
    return _header()[2][name]


def struct_ctype(name: str):
    """The same field list as a ctypes.Structure class, for the few structs that are passed one at a time with byref()."""
    fields = []
    for field in struct_dtype(name).names:
        base, shape = struct_dtype(name)[field].subdtype or (struct_dtype(name)[field], ())
        kind = C.c_void_p if (base.metadata or {}).get("pointer") else np.ctypeslib.as_ctypes_type(base)
        for n in reversed(shape):
            kind = kind * n
        fields.append((field, kind))
    return type(name, (C.Structure,), {"_fields_": fields})


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
