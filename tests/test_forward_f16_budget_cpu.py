"""No GPU: the fp16 forward budgets (tests/forward_f16_budget.py) and the HH_DTYPE_F16 handle as far as the host goes."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import forward_budget as fb
import forward_f16_budget as f16
from oracle import forward as ofw


def test_bf16_emulation_fails_every_fp16_budget():
    """The budgets can tell the two formats apart: on every output of every lattice case the bf16-storage emulation is over the fp16
    budget in all five figures.  (An engine left multiplying in bf16 -- all of it or one kernel family -- cannot pass as fp16.)
    Measured: least bf16 figure / allowed fp16 figure 3.84 (rms), 3.77 (row), 3.65 (col), 3.77 (img), 2.11 (max)."""
    least = {k: float("inf") for k in fb.FIGURES}
    for case in f16.LATTICE_F16:
        kind, Cw, B, H, W = case
        seed, iseed = f16.seeds(case)
        cls = kind == "cls"
        ref, _ = f16.tensors_f16((B, H, W), Cw, seed, iseed, cls)
        emu_bf16 = fb._forward(fb.images((B, H, W), iseed), fb.state_dict(Cw, seed, cls), "bf16", cls)
        for name in f16.OUTPUTS[kind]:
            fig = fb.figures(emu_bf16[name], ref[name])
            allowed = f16.budget_f16(name, (B, H, W), Cw, seed, iseed, cls)
            for k in fb.FIGURES:
                ratio = fig[k][0] / allowed[k]
                least[k] = min(least[k], ratio)
                assert ratio > 1, f"{f16.case_id(case)} {name}: the bf16 emulation's {k} {fig[k][0]:.5f} is within the fp16 budget {allowed[k]:.5f}"
            with pytest.raises(AssertionError):
                fb.check(emu_bf16[name], ref[name], allowed, "bf16 emulation under the fp16 budget")
    print("least bf16 figure / allowed fp16 figure:", {k: round(v, 2) for k, v in least.items()})


def test_fp16_patch_leaves_the_oracle_as_it_was():
    """forward_f16 swaps oracle.forward._q for the duration of a call: afterwards storage="fp32" and storage="bf16" give the bits they
    gave before, also when the emulation raised."""
    shape = (1, 32, 32)
    sd, x = fb.state_dict(32, 1), fb.images(shape, 7)
    q = ofw._q
    before = {s: fb._forward(x, sd, s, False) for s in ("fp32", "bf16")}
    emu = f16.forward_f16(x, sd)
    assert ofw._q is q
    with pytest.raises(KeyError):
        f16.forward_f16(x, {})  # a forward that fails inside the patched walk
    assert ofw._q is q
    after = {s: fb._forward(x, sd, s, False) for s in ("fp32", "bf16")}
    for s in before:
        for name in before[s]:
            assert np.array_equal(before[s][name], after[s][name]), (s, name)
    # and the emulation is a third thing: between the two (closer to fp32 than bf16 is), on the fp16 grid
    for name in ("hm_q", "hm_h", "tags"):
        e16 = fb.figures(emu[name], before["fp32"][name])["rms"][0]
        ebf = fb.figures(before["bf16"][name], before["fp32"][name])["rms"][0]
        assert 0 < e16 < ebf / 4, (name, e16, ebf)
    stem = torch.from_numpy(emu["stem#0"])
    assert torch.equal(stem, stem.to(torch.float16).to(torch.float32))


def _names(lib, h):
    return [lib.hh_param_name(h, i).decode() for i in range(lib.hh_num_params(h))]


def test_c_abi_accepts_the_fp16_dtype_without_a_gpu(pkg):
    """hh_create / hh_create_classifier with HH_DTYPE_F16 = 3: the same plan as bf16 (parameter names, FLOPs, a hazard-free schedule);
    other codes and debug switches that reach a bf16-only kernel are refused with a message; the ABI version stays 3."""
    lib = pkg._lib.load()
    BF16, F16 = 1, 3
    assert lib.hh_abi_version() == 3
    made = []
    try:
        for create, args in ((lib.hh_create, (17, 32)), (lib.hh_create, (17, 48)), (lib.hh_create_classifier, (32, 1000))):
            h16, hbf = create(*args, F16), create(*args, BF16)
            assert h16, lib.hh_last_error().decode()
            assert hbf, lib.hh_last_error().decode()
            h16, hbf = C.c_void_p(h16), C.c_void_p(hbf)
            made += [h16, hbf]
            assert lib.hh_debug_check_plan(h16) == 0, lib.hh_last_error().decode()
            assert _names(lib, h16) == _names(lib, hbf)
            for shape in ((1, 64, 64), (32, 512, 512), (3, 96, 160)):
                assert lib.hh_forward_flops(h16, *shape) == lib.hh_forward_flops(hbf, *shape) > 0
        assert not lib.hh_create(17, 32, 7)
        msg = lib.hh_last_error().decode()
        assert "HH_DTYPE_BF16" in msg and "HH_DTYPE_FP8" in msg and "HH_DTYPE_F16" in msg, msg
        assert not lib.hh_create_classifier(32, 1000, 2)  # the classifier has no fp8 form
        assert "HH_DTYPE_F16" in lib.hh_last_error().decode()
        for env, word in (({"HH_NO_STEM_FUSED": "1"}, "HH_NO_STEM_FUSED"), ({"HH_BB32": "tile"}, "HH_BB32")):
            os.environ.update(env)
            try:
                refused = (lib.hh_create(17, 32, F16), lib.hh_last_error().decode(), lib.hh_create_classifier(32, 10, F16), lib.hh_last_error().decode())
                ok = lib.hh_create(17, 32, BF16)  # the switch itself stays valid for bf16
            finally:
                for k in env:
                    del os.environ[k]
            assert ok
            made.append(C.c_void_p(ok))
            assert not refused[0] and word in refused[1] and "fp16" in refused[1], refused
            assert not refused[2] and word in refused[3], refused
        # hh_calibrate belongs to fp8 handles (the handle's type is looked at before the images are)
        host = np.zeros(3 * 32 * 32, np.float32)
        assert lib.hh_calibrate(made[0], host.ctypes.data, 1, 32, 32, 1, None) != 0
        assert "not an fp8 handle" in lib.hh_last_error().decode()
    finally:
        for h in made:
            lib.hh_destroy(h)


def test_python_modules_take_the_fp16_dtype(pkg):
    net = pkg.HigherHRNet(17, 32, dtype="fp16")
    assert net.engine_dtype == "fp16" and pkg.HigherHRNet.DTYPES["fp16"] == 3
    with pytest.raises(ValueError, match="fp17"):
        pkg.HigherHRNet(17, 32, dtype="fp17")
    cls = pkg.ClassificationHRNet(32, 10, dtype="fp16")
    assert cls.engine_dtype == "fp16" and pkg.ClassificationHRNet(32, 10).engine_dtype == "bf16"
    with pytest.raises(ValueError):
        pkg.ClassificationHRNet(32, 10, dtype="fp8")
    # set_engine_dtype: a new handle of the other type, weights to be folded again; an unknown name leaves the net as it was
    lib = pkg._lib.load()
    h = net._h
    net._dirty = False
    net.set_engine_dtype("fp16")
    assert net._h == h and not net._dirty  # the same type: nothing to do
    net.set_engine_dtype("bf16")
    assert net.engine_dtype == "bf16" and net._dirty and lib.hh_debug_check_plan(net._h) == 0
    with pytest.raises(ValueError):
        net.set_engine_dtype("int8")
    assert net.engine_dtype == "bf16"
