"""The CPU side of the training-precision switch: names are checked where they are given, and the module's checkpoint entry has the
reference's format ({"scalers": {name: GradScaler.state_dict()}}, base/module.py:109-127)."""
import ctypes
import importlib
import warnings

import pytest
import torch

from conftest import PKG


def _km():
    return importlib.import_module(PKG + ".keypoints.model")


def test_set_train_precision_rejects_unknown_names(pkg):
    net = pkg.HigherHRNet(17, 32)
    assert net.train_precision == "bf16"
    for name in ("fp16", "bf16"):
        net.set_train_precision(name)
        assert net.train_precision == name
    for bad in ("fp32", "float16", "", None, 16):
        with pytest.raises(ValueError, match="set_train_precision"):
            net.set_train_precision(bad)
    assert net.train_precision == "bf16"
    ops = importlib.import_module(PKG + ".keypoints.train_ops")
    assert set(ops.PRECISION_DTYPES) == set(net.TRAIN_PRECISIONS) and ops.PRECISION_DTYPES["fp16"] is torch.float16
    assert {ops.ACT_DTYPES[torch.bfloat16], ops.ACT_DTYPES[torch.float16]} == {0, 1}  # HH_ACT_BF16, HH_ACT_F16


def test_keypoints_module_rejects_unknown_precisions_and_keeps_the_scaler_format(pkg):
    km = _km()
    net = pkg.HigherHRNet(17, 32)
    model = km.KeypointsModel(net)
    opt = torch.optim.SGD(net.parameters(), lr=0.0)
    for bad in ("fp32", "amp", None):
        with pytest.raises(ValueError, match="precision"):
            km.KeypointsModule(model, None, opt, precision=bad)
    module = km.KeypointsModule(model, None, opt)
    assert module.precision == "bf16" and module.scalers == {} and module.state_dict() == {"scalers": {}} and net.train_precision == "bf16"
    module.load_state_dict({"scalers": {}})
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # (without a GPU torch says that it disables the scaler; its state is then empty on both sides)
        module = km.KeypointsModule(model, None, opt, precision="fp16")
        assert net.train_precision == "fp16" and set(module.scalers) == {"optim"} and type(module.scalers["optim"]) is torch.amp.GradScaler
        state = module.state_dict()
        assert set(state) == {"scalers"} and set(state["scalers"]) == {"optim"}
        assert set(state["scalers"]["optim"]) == set(torch.amp.GradScaler("cuda").state_dict())
    with pytest.raises(KeyError):
        module.load_state_dict({"scalers": {}})  # like the reference: every scaler's state must be there


def test_dt_entry_points_are_declared_exported_and_bound(pkg):
    lib = pkg._lib.load()
    names = [n for n in pkg._lib.exported_symbols() if n.endswith("_dt")]
    assert len(names) == 13 and all(n[:-3] in pkg._lib.exported_symbols() for n in names)
    for n in names:
        fn, old = getattr(lib, n), getattr(lib, n[:-3])
        assert list(fn.argtypes) == [ctypes.c_int] + list(old.argtypes) and fn.restype is old.restype, n
    header = open(pkg._lib.HEADER).read()
    assert "#define HH_ACT_BF16 0" in header and "#define HH_ACT_F16 1" in header and "#define HH_ABI_VERSION 3" in header
    assert (pkg._lib.ACT_BF16, pkg._lib.ACT_F16) == (0, 1)
