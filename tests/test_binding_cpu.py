"""The Python binding's policies, each in one place (`_lib.py`): ctypes signatures, constants and descriptor-struct layouts derived
from include/hhrnet.h, and `launch`, the one way device work is enqueued (device guard, that device's current stream last, status
checked).  No GPU needed: the device guard and the stream lookup are replaced by recorders."""
import contextlib
import ctypes as C
import glob
import importlib
import os
import types

import numpy as np
import pytest
import torch

from conftest import PKG, REPO


# ---------------------------------------------------------------- signatures
def test_every_exported_symbol_has_a_derived_signature(pkg):
    sigs = pkg._lib.signatures()
    names = pkg._lib.exported_symbols()
    assert len(names) > 100 and set(names) == set(sigs)
    lib = pkg._lib.load()
    for name in names:
        fn = getattr(lib, name)
        assert fn.restype is sigs[name][0] and list(fn.argtypes) == sigs[name][1], name


def test_signatures_written_out(pkg):
    i, i64, f, d, vp, cp = C.c_int, C.c_int64, C.c_float, C.c_double, C.c_void_p, C.c_char_p
    sigs = pkg._lib.signatures()
    assert sigs["hh_last_error"] == (cp, [])
    assert sigs["hh_create"] == (vp, [i, i, i])
    assert sigs["hh_destroy"] == (None, [vp])
    assert sigs["hh_workspace_bytes"] == (i64, [vp])
    assert sigs["hh_forward_flops"] == (d, [vp, i, i, i])
    assert sigs["hh_load_weights"] == (i, [vp, cp, vp, vp, i])  # `const char *name` stays a string, every other pointer is void*
    # (x, int64_t P, C, gamma, beta, float eps, res, relu, y, mean, invstd, scratch, stream)
    assert sigs["hh_bn_train_forward"] == (i, [vp, i64, i, vp, vp, f, vp, i, vp, vp, vp, vp, vp])
    assert sigs["hh_bn_train_forward_dt"] == (i, [i] + sigs["hh_bn_train_forward"][1])
    # (maps_dev, maps_host, n, image, H, W, lut, canvas, Hc, Wc, long long pitch, scratch, stream)
    assert sigs["hh_heatmap_panels_u8"] == (i, [vp, vp, i, vp, i, i, vp, vp, i, i, i64, vp, vp])
    assert sigs["hh_conv_config"] == (i, [i, vp])  # `int out[7]` is a pointer
    assert sigs["hh_profile_get"] == (i, [vp, i, vp, vp, vp, vp, vp, vp])
    assert sigs["hh_decoder_create"] == (vp, [i, i, d, d])
    assert C.sizeof(i64) == 8 and C.sizeof(i) == 4


def test_constants_come_from_the_header(pkg):
    header = open(pkg._lib.HEADER).read()
    _, consts = pkg._lib.parse_header(header)
    assert (consts["HH_ABI_VERSION"], consts["HH_ACT_BF16"], consts["HH_ACT_F16"]) == (3, 0, 1)
    assert (pkg._lib.ACT_BF16, pkg._lib.ACT_F16) == (consts["HH_ACT_BF16"], consts["HH_ACT_F16"])
    sigs, consts = pkg._lib.parse_header(header.replace("#define HH_ACT_F16 1", "#define HH_ACT_F16 7"))
    assert consts["HH_ACT_F16"] == 7 and set(sigs) == set(pkg._lib.exported_symbols())


@pytest.mark.parametrize("bad", [
    "int hh_new_thing(struct hh_image_desc d, void *stream);",   # a struct by value
    "int hh_new_thing(size_t n, void *stream);",                  # an integer type the table of kinds does not list
    "hh_image_desc hh_new_thing(int n);",                         # an unknown return type
    "int hh_new_thing(int (*callback)(int), void *stream);",      # a function pointer
    "int hh_new_thing(int n, ...);",                              # variadic
    "int hh_new_thing(int);",                                     # a parameter without a name
    "static inline int hh_new_thing(int n) { return n; }",        # not a prototype at all
    "int hh_abi_version(void);",                                  # declared twice
])
def test_unparseable_prototype_raises(pkg, bad):
    header = open(pkg._lib.HEADER).read()
    marker = "int hh_abi_version(void);"
    assert header.count(marker) == 1
    with pytest.raises(pkg._lib.HHError, match="hh_new_thing|hh_abi_version"):
        pkg._lib.parse_header(header.replace(marker, marker + "\n" + bad))
    # the same text with a well-formed addition parses, multi-line and array parameters included
    good = "int hh_new_thing(const float *x, int64_t n,\n                 const double m[6], long long pitch, float eps, void *stream);"
    sigs, _ = pkg._lib.parse_header(header.replace(marker, marker + "\n" + good))
    assert sigs["hh_new_thing"] == (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_float, C.c_void_p])


# ---------------------------------------------------------------- descriptor structs
SIZES = {"hh_image_desc": 64, "hh_train_desc": 272, "hh_mosaic_tile": 24, "hh_mosaic_desc": 112, "hh_crowd_mask_desc": 24, "hh_crowd_seg_desc": 24,
         "hh_render_prim": 32, "hh_render_desc": 48, "hh_panel_map": 40, "hh_jpeg_desc": 64, "hh_jpeg_stream_info": 112, "hh_jpeg_segment": 32,
         "hh_jpeg_dec_desc": 64, "hh_jpeg_window": 16, "hh_jpeg_win_desc": 80, "hh_jpeg_window_counts": 48, "hh_coco_tables": 136,
         "hh_track_params": 592, "hh_crop_desc": 56, "hh_xent_result": 16, "hh_optim_tensor": 56, "hh_optim_group": 56, "hh_ema_row": 24,
         "hh_scale_src": 48}


def _structs(pkg, text=None):
    return pkg._lib.parse_structs(open(pkg._lib.HEADER).read() if text is None else text)


def _layout(dt):
    """[(field, offset, numpy kind string with the array shape)] of a struct dtype, in declaration order."""
    return [(n, dt.fields[n][1], (dt[n].subdtype[0].str + str(list(dt[n].shape))) if dt[n].subdtype else dt[n].str) for n in dt.names]


def test_struct_sizes_written_out(pkg):
    structs = _structs(pkg)
    assert {n: dt.itemsize for n, dt in structs.items()} == SIZES  # ABI version 3: every struct of the header, no other
    assert all(pkg._lib.struct_dtype(n) == dt for n, dt in structs.items())


def test_struct_fields_written_out(pkg):
    S = _structs(pkg)
    # a nested struct
    assert _layout(S["hh_mosaic_tile"]) == [("image_offset", 0, "<i8"), ("mask_offset", 8, "<i8"), ("h", 16, "<i4"), ("w", 20, "<i4")]
    assert S["hh_mosaic_desc"].names == ("tile", "canvas_image_offset", "canvas_mask_offset")
    assert S["hh_mosaic_desc"]["tile"].subdtype == (S["hh_mosaic_tile"], (4,))
    assert [S["hh_mosaic_desc"].fields[n][1] for n in S["hh_mosaic_desc"].names] == [0, 96, 104]
    assert S["hh_jpeg_win_desc"].names == ("d", "window") and S["hh_jpeg_win_desc"]["d"] == S["hh_jpeg_dec_desc"]
    assert S["hh_jpeg_win_desc"].fields["window"] == (S["hh_jpeg_window"], 64)
    # a 2-d array bounded by a macro
    assert _layout(S["hh_train_desc"]) == [("image_offset", 0, "<i8"), ("mask_offset", 8, "<i8"), ("h", 16, "<i4"), ("w", 20, "<i4"), ("flip", 24, "<i4"),
                                           ("reserved", 28, "<i4"), ("image_dst_to_src", 32, "<f8[6]"), ("mask_dst_to_src", 80, "<f8[4, 6]")]
    # pointers
    assert _layout(S["hh_optim_tensor"]) == [("param", 0, "<u8"), ("grad", 8, "<u8"), ("state0", 16, "<u8"), ("state1", 24, "<u8"), ("step", 32, "<u8"),
                                             ("numel", 40, "<i8"), ("group", 48, "<i4"), ("reserved", 52, "<i4")]
    assert _layout(S["hh_panel_map"]) == [("src", 0, "<u8"), ("src2", 8, "<u8"), ("h", 16, "<i4"), ("w", 20, "<i4"), ("kind", 24, "<i4"),
                                          ("flags", 28, "<i4"), ("oy", 32, "<i4"), ("ox", 36, "<i4")]
    # small members, and tail padding (48 bytes for 44 of fields)
    assert _layout(S["hh_render_prim"]) == [("cx", 0, "<i4"), ("cy", 4, "<i4"), ("A", 8, "<u2"), ("B", 10, "<u2"), ("c", 12, "<f4"), ("s", 16, "<f4"),
                                            ("rgb", 20, "|u1[3]"), ("kind", 23, "|u1"), ("x0", 24, "<i2"), ("y0", 26, "<i2"), ("x1", 28, "<i2"),
                                            ("y1", 30, "<i2")]
    assert _layout(S["hh_scale_src"])[-3:] == [("h", 32, "<i4"), ("w", 36, "<i4"), ("weight", 40, "<f4")]
    # the ctypes form of the same list
    T = pkg._lib.struct_ctype("hh_coco_tables")
    assert C.sizeof(T) == 136 and [(n, getattr(T, n).offset) for n, _ in T._fields_] == [(n, S["hh_coco_tables"].fields[n][1]) for n in S["hh_coco_tables"].names]
    assert all(k is C.c_void_p for _, k in T._fields_[:13]) and T._fields_[-1][1] is C.c_int32 * 2


def test_struct_layouts_equal_the_compilers(pkg, tmp_path):
    """sizeof and every offsetof, as the host C compiler reports them for include/hhrnet.h, against the derived dtypes."""
    import shutil
    import subprocess
    cc = next((c for c in ("cc", "gcc", "/opt/rocm/lib/llvm/bin/clang", "/opt/rocm/llvm/bin/clang") if shutil.which(c)), None)
    assert cc is not None, "no host C compiler (cc, gcc, ROCm's clang)"
    structs = _structs(pkg)
    lines = ['#include <stddef.h>', '#include <stdio.h>', f'#include "{pkg._lib.HEADER}"', "int main(void) {"]
    for name, dt in structs.items():
        lines.append(f'    printf("{name} %zu", sizeof({name}));')
        lines += [f'    printf(" {f}=%zu", offsetof({name}, {f}));' for f in dt.names]
        lines.append('    printf("\\n");')
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines + ["    return 0;", "}", ""]))
    subprocess.run([cc, "-std=c99", str(src), "-o", str(tmp_path / "layout")], check=True)
    out = subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout
    want = "".join(f"{n} {dt.itemsize}" + "".join(f" {f}={dt.fields[f][1]}" for f in dt.names) + "\n" for n, dt in structs.items())
    assert len(structs) == len(SIZES) and out == want


def test_struct_parser_notices_edits(pkg):
    header = open(pkg._lib.HEADER).read()
    a, b = "    int32_t h, w;\n    int32_t prim_offset, prim_count;\n", "    int32_t prim_offset, prim_count;\n    int32_t h, w;\n"
    assert header.count(a) == 1  # (inside hh_render_desc)
    was, now = _structs(pkg)["hh_render_desc"], _structs(pkg, header.replace(a, b))["hh_render_desc"]
    assert was.itemsize == now.itemsize == 48
    assert [was.fields[n][1] for n in ("h", "w", "prim_offset", "prim_count")] == [16, 20, 24, 28]
    assert [now.fields[n][1] for n in ("h", "w", "prim_offset", "prim_count")] == [24, 28, 16, 20]
    stages = "#define HH_TRAIN_MAX_STAGES 4"
    assert header.count(stages) == 1
    assert _structs(pkg, header.replace(stages, "#define HH_TRAIN_MAX_STAGES 5"))["hh_train_desc"].itemsize == 272 + 48


@pytest.mark.parametrize("bad", [
    "size_t n;",                              # a type the table of kinds does not list
    "struct hh_image_desc d;",                # a struct that is not spelled as a parsed hh_* typedef
    "hh_ema_row row;",                        # a struct defined further down
    "int flags : 3;",                         # a bit-field
    "union { int i; float f; } u;",           # a union
    "int (*callback)(int);",                  # a function pointer
    "double m[HH_NO_SUCH_LIMIT];",            # a bound that is no parsed macro
    "double m[2 * 3];",                       # a bound that is an expression
    "double m[0];",                           # no room
    "int h;",                                 # a name twice
])
def test_unparseable_struct_body_raises(pkg, bad):
    header = open(pkg._lib.HEADER).read()
    marker = "typedef struct hh_image_desc {"
    assert header.count(marker) == 1
    added = "typedef struct hh_new_thing {\n    int h, w;\n    %s\n} hh_new_thing;\n"
    with pytest.raises(pkg._lib.HHError, match="hh_new_thing"):
        pkg._lib.parse_header(header.replace(marker, added % bad + marker))
    # the same text with a well-formed addition parses: pointers, macro-bounded and 2-d arrays, a nested struct, several names per line
    good = "const float *src, *const *list;\n    long long at[HH_TRAIN_MAX_STAGES][2];\n    hh_image_desc image[2];\n    uint8_t a, b[3];"
    dt = _structs(pkg, header.replace("typedef struct hh_train_desc {", added % good + "typedef struct hh_train_desc {"))["hh_new_thing"]
    assert _layout(dt)[:5] == [("h", 0, "<i4"), ("w", 4, "<i4"), ("src", 8, "<u8"), ("list", 16, "<u8"), ("at", 24, "<i8[4, 2]")]
    assert dt.fields["image"][1] == 88 and dt.fields["a"][1] == 216 and dt.fields["b"][1] == 217 and dt.itemsize == 224


def test_no_module_restates_a_table():
    """The descriptor tables and their sizes are written in include/hhrnet.h alone: outside _lib.py the package has no dtype literal,
    no ctypes field list and no itemsize assertion."""
    import re
    files = [f for f in glob.glob(os.path.join(REPO, PKG, "**", "*.py"), recursive=True) if os.path.basename(f) != "_lib.py"]
    assert len(files) > 20
    hits = [(os.path.relpath(f, REPO), m.group(0)) for f in files
            for m in re.finditer(r"np\.dtype\(\s*\[|_fields_\s*=|assert[^\n]*itemsize\s*==|ctypes\.Structure|C\.Structure", open(f).read())]
    assert hits == []


# ---------------------------------------------------------------- launch
class Recorder:
    """Stands in for torch.cuda.device / torch.cuda.current_stream: `active` is the stack of guarded devices, `log` every event."""

    def __init__(self, monkeypatch):
        self.active, self.log = [], []
        monkeypatch.setattr(torch.cuda, "device", self.device)
        monkeypatch.setattr(torch.cuda, "current_stream", self.current_stream)

    @contextlib.contextmanager
    def device(self, dev):
        self.active.append(dev)
        self.log.append(("enter", dev))
        try:
            yield
        finally:
            self.log.append(("exit", dev))
            self.active.pop()

    @staticmethod
    def handle(dev) -> int:
        return 0x1000 + sum(map(ord, str(dev)))

    def current_stream(self, dev=None):
        self.log.append(("stream", dev, tuple(self.active)))
        return types.SimpleNamespace(cuda_stream=self.handle(dev))

    def entry_point(self, name, status=0):
        def fn(*args):
            self.log.append(("call", name, args, tuple(self.active)))
            return status
        return fn

    def calls(self, name):
        return [e for e in self.log if e[0] == "call" and e[1] == name]


def test_launch_guards_the_device_and_appends_its_stream(pkg, monkeypatch):
    rec = Recorder(monkeypatch)
    dev = torch.device("cuda", 1)
    assert pkg._lib.launch(dev, rec.entry_point("hh_fake"), 11, None, 2.5) is None
    kinds = [e[0] for e in rec.log]
    assert kinds == ["enter", "stream", "call", "exit"]
    assert rec.log[1] == ("stream", dev, (dev,))  # the stream is that device's, read inside the guard
    assert rec.log[2] == ("call", "hh_fake", (11, None, 2.5, Recorder.handle(dev)), (dev,))
    assert rec.active == []


def test_launch_raises_the_librarys_last_error(pkg, monkeypatch):
    rec = Recorder(monkeypatch)
    lib = pkg._lib.load()
    assert lib.hh_heatmap_table_size(1.0, None, None) != 0  # a host-side refusal: sets the thread's last error
    text = lib.hh_last_error().decode()
    assert text == "hh_heatmap_table_size: null pointer"
    with pytest.raises(pkg._lib.HHError) as e:
        pkg._lib.launch("cuda:0", rec.entry_point("hh_fake", status=1))
    assert str(e.value) == text and rec.active == []


def test_ptr(pkg):
    t = torch.zeros(3)
    assert pkg._lib.ptr(None) is None and pkg._lib.ptr(t) == t.data_ptr()


# ---------------------------------------------------------------- one place
def test_only_the_binding_names_the_stream_handle():
    files = glob.glob(os.path.join(REPO, PKG, "**", "*.py"), recursive=True)
    assert len(files) > 20
    hits = [os.path.relpath(f, REPO) for f in files if "cuda_stream" in open(f).read()]
    assert hits == [os.path.join(PKG, "_lib.py")]


# ---------------------------------------------------------------- the sites that had no guard
def test_flip_tta_launches_under_its_tensors_device(pkg, monkeypatch):
    """forward_tta(use_flip=True) on tiny CPU stand-ins with a recording library: hh_flip_images and both hh_flip_merge calls run
    inside the guard of x.device, each with that device's stream as its last argument."""
    rec = Recorder(monkeypatch)
    model_mod = importlib.import_module(PKG + ".keypoints.model")
    K, B, H, W = 17, 2, 8, 8
    net = types.SimpleNamespace(num_kpts=K, forward_raw=lambda x2: (torch.zeros(x2.shape[0], 2 * K, H // 4, W // 4), torch.zeros(x2.shape[0], K, H // 2, W // 2)))
    m = object.__new__(model_mod.InferenceKeypointsModel)
    m.net, m.use_flip, m._perm = net, True, np.arange(K, dtype=np.int32)
    m._lib = types.SimpleNamespace(hh_flip_images=rec.entry_point("hh_flip_images"), hh_flip_merge=rec.entry_point("hh_flip_merge"))
    x = torch.zeros(B, 3, H, W)
    hms, tags = m.forward_tta(x)
    assert len(hms) == 2 and len(tags) == 2
    assert len(rec.calls("hh_flip_images")) == 1 and len(rec.calls("hh_flip_merge")) == 2
    for _, name, args, active in rec.calls("hh_flip_images") + rec.calls("hh_flip_merge"):
        assert active == (x.device,), name
        assert args[-1] == Recorder.handle(x.device), name


def test_dirty_module_finalizes_under_its_inputs_device(pkg, monkeypatch):
    """_check_input of a module with stale weights: hh_finalize (which allocates and uploads on the current device) is reached inside
    the guard of the input's device."""
    rec = Recorder(monkeypatch)
    arch = importlib.import_module(PKG + ".keypoints.architectures.higher_hrnet")
    dev = torch.device("cuda", 1)

    class Images:  # what _check_input reads of its input
        is_cuda, device, shape = True, dev, (1, 3, 32, 32)
        contiguous = float = lambda self: self
        dim = lambda self: 4  # noqa: E731

    mod = types.SimpleNamespace(training=False, _dirty=True, _h=None, state_dict=dict,
                                _lib=types.SimpleNamespace(hh_finalize=rec.entry_point("hh_finalize")))
    mod.sync_weights = lambda: arch.EngineModule.sync_weights(mod)
    images = Images()
    assert arch.EngineModule._check_input(mod, images) is images and mod._dirty is False
    (call,) = rec.calls("hh_finalize")
    assert call[3] == (dev,) and rec.active == []
