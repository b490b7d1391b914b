"""The stage-0 -> 1 transition as ONE dual-output launch (conv_mfma.hip, DUAL: the 256 -> 32 stride-1 conv and the 256 -> 64 stride-2
conv over one staged patch) against the two-launch plan it replaces (HH_NO_TRANS_DUAL=1): the same bits at both forward outputs, in
both lane modes, on a freshly poisoned workspace, for bf16 and fp16 handles; W48 keeps the two launches.  The plan checks at the end
need no GPU."""
import contextlib
import ctypes as C
import os

import pytest
import torch

DEV = "cuda:0"
# (B, H, W) of the input; the stage-0 map is H/4 x W/4 and the dual launch tiles it 8 x 32 (secondary: 4 x 16):
#   32x32 -> 8x8: a single partial tile with a 4x4 stride-2 output (B = 1 and B = 3)
#   64x64 -> 16x16;  96x160 -> 24x40: ragged in both tile directions;  128x128 -> 32x32: full tiles, image borders on every side
# In this order every shape grows the reserved workspace, so an HH_POISON_WS=1 handle gets a freshly poisoned one for every run.
SHAPES = ((1, 32, 32), (3, 32, 32), (1, 64, 64), (1, 96, 160), (1, 128, 128))
OFF = {"HH_NO_TRANS_DUAL": "1"}
POISON = {"HH_POISON_WS": "1"}
CFG_TRANS_DUAL = 108  # kernels.h HH_CFG_TRANS_DUAL


@contextlib.contextmanager
def _env(env):
    os.environ.update(env)
    try:
        yield
    finally:
        for k in env:
            del os.environ[k]


def _net(pkg, C_, seed, env=None, dtype="bf16", lanes=1):
    with _env(env or {}):
        net = pkg.HigherHRNet(17, C_, dtype=dtype)
    sd = {k: torch.from_numpy(pkg.synth.synth_param(k, v.shape, seed)) for k, v in net.state_dict().items()}
    net.load_state_dict(sd)
    net = net.to(DEV).eval()
    pkg._lib.load().hh_set_multi_lane(net._h, lanes)
    return net


def _same(a, b, what):
    for u, v, name in zip(a, b, ("init_heatmaps", "deconv_heatmaps")):
        assert u.shape == v.shape, (what, name)
        assert torch.isfinite(u).all(), f"{what} {name}: not finite (a value no kernel stored?)"
        if not torch.equal(u, v):
            d = u != v
            raise AssertionError(f"{what} {name}: {int(d.sum())} of {d.numel()} values differ, first at {tuple(d.nonzero()[0].tolist())}")


def _compare(pkg, C_, dtype, shapes, seed):
    """Per lane mode one handle of the default plan with a poisoned workspace, against the two-launch plan in the same lane mode."""
    lib = pkg._lib.load()
    plain = _net(pkg, C_, seed, OFF, dtype)
    for lanes in (1, 0):
        dual = _net(pkg, C_, seed, POISON, dtype, lanes)
        lib.hh_set_multi_lane(plain._h, lanes)
        for i, shape in enumerate(shapes):
            x = torch.from_numpy(pkg.synth.synth_images(*shape, 80 + i)).to(DEV)
            ref = [t.clone() for t in plain.forward_raw(x)]
            _same(dual.forward_raw(x), ref, f"W{C_} {dtype} {shape} lanes={lanes}")


@pytest.mark.gpu
def test_dual_transition_equals_the_two_launches(pkg):
    _compare(pkg, 32, "bf16", SHAPES, 11)


@pytest.mark.gpu
def test_dual_transition_equals_the_two_launches_fp16(pkg):
    _compare(pkg, 32, "fp16", SHAPES, 12)


@pytest.mark.gpu
def test_w48_keeps_the_two_launch_plan_exact(pkg):
    """48 / 96 couts do not fit the dual kernel: the default W48 plan is the two-launch one, with and without the switch."""
    _compare(pkg, 48, "bf16", ((1, 32, 32), (2, 96, 160)), 13)


@pytest.mark.gpu
def test_dual_launch_is_profiled_under_its_own_config(pkg):
    lib = pkg._lib.load()
    x = torch.from_numpy(pkg.synth.synth_images(1, 64, 64, 3)).to(DEV)
    cfg, flops, nbytes, ms, kms, name = C.c_int(), C.c_double(), C.c_double(), C.c_float(), C.c_float(), C.c_char_p()
    seen = {}
    for what, env in (("dual", {}), ("two launches", OFF)):
        net = _net(pkg, 32, 1, env)
        pkg._lib.check(lib.hh_profile_enable(net._h, 1))
        try:
            net.forward_raw(x)
            torch.cuda.synchronize()
            seen[what] = []
            for i in range(lib.hh_profile_count(net._h)):
                pkg._lib.check(lib.hh_profile_get(net._h, i, C.byref(cfg), C.byref(flops), C.byref(nbytes), C.byref(ms), C.byref(kms), C.byref(name)))
                seen[what].append((cfg.value, flops.value))
        finally:
            lib.hh_profile_enable(net._h, 0)
    dual = [f for c, f in seen["dual"] if c == CFG_TRANS_DUAL]
    assert len(dual) == 1 and not [c for c, _ in seen["two launches"] if c == CFG_TRANS_DUAL]
    assert len(seen["dual"]) == len(seen["two launches"]) - 1
    # 2 * (16x16 px * 256 * 32 + 8x8 px * 256 * 64) * 9 taps: the two convs' FLOPs in one record
    assert dual[0] == 2.0 * (16 * 16 * 256 * 32 + 8 * 8 * 256 * 64) * 9


# ---- plan checks (no GPU)
SWITCHES = ({}, {"HH_FULL_JOIN": "1"}, {"HH_KEEP_WAITS": "1"}, {"HH_NO_JUNC_PAIR": "1"}, {"HH_NO_FUSION_MERGE": "1", "HH_FULL_JOIN": "1"})


def test_plan_checker_with_and_without_the_dual_transition(pkg):
    lib = pkg._lib.load()
    for dual in ({}, OFF):
        for sw in SWITCHES:
            env = dict(dual, **sw)
            with _env(env):
                nets = (pkg.HigherHRNet(17, 32), pkg.HigherHRNet(17, 32, dtype="fp16"), pkg.HigherHRNet(17, 48), pkg.HigherHRNet(5, 32),
                        pkg.ClassificationHRNet(32, 10))
            for net in nets:
                assert lib.hh_debug_check_plan(net._h) == 0, (env, lib.hh_last_error().decode())


def test_dual_transition_keeps_the_flop_count(pkg):
    lib = pkg._lib.load()
    for C_, dtype in ((32, "bf16"), (32, "fp16"), (48, "bf16")):
        dual = pkg.HigherHRNet(17, C_, dtype=dtype)
        with _env(OFF):
            plain = pkg.HigherHRNet(17, C_, dtype=dtype)
        for B, H, W in ((1, 512, 512), (32, 512, 512), (1, 32, 32), (5, 352, 416)):
            a = lib.hh_forward_flops(dual._h, B, H, W)
            b = lib.hh_forward_flops(plain._h, B, H, W)
            assert a == b and a > 0, (C_, dtype, B, H, W, a, b)
    w32 = pkg.HigherHRNet(17, 32)
    for B in (1, 32):  # 46.2034 GMAC per 512 x 512 image
        assert lib.hh_forward_flops(w32._h, B, 512, 512) == 2 * 46203404288.0 * B
