"""The Python binding's two policies, each in one place (`_lib.py`): ctypes signatures derived from include/hhrnet.h, and `launch`,
the one way device work is enqueued (device guard, that device's current stream last, status checked).  No GPU needed: the device
guard and the stream lookup are replaced by recorders."""
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
