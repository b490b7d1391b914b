"""-m gpu: output 0 of every fusion layer as one fusion_up.hip launch (1x1 terms once per low-resolution pixel, kept in LDS) gives
the bits of the launch chain it replaces (HH_NO_FUSED_UPSUM=1: a conv_mfma 1x1 per source + upadd_kernel) -- on both lane modes,
on ragged and single-tile shapes, on fresh and poisoned memory, and the same bits on every call."""
import contextlib
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = ((2, 128, 128), (4, 512, 512), (5, 352, 416), (3, 96, 160), (1, 32, 64), (1, 64, 32))


@contextlib.contextmanager
def _env(env):
    os.environ.update(env)
    try:
        yield
    finally:
        for k in env:
            del os.environ[k]


def _net(pkg, C, seed, env=None):
    with _env(env or {}):
        net = pkg.HigherHRNet(17, C)
    sd = {k: torch.from_numpy(pkg.synth.synth_param(k, v.shape, seed)) for k, v in net.state_dict().items()}
    net.load_state_dict(sd)
    return net.to(DEV).eval()


def _same(a, b, what):
    for u, v, name in zip(a, b, ("init_heatmaps", "deconv_heatmaps")):
        assert u.shape == v.shape, (what, name)
        if not torch.equal(u, v):
            d = (u != v) | (u.isnan() != v.isnan())
            raise AssertionError(f"{what} {name}: {int(d.sum())} of {d.numel()} values differ, first at {tuple(d.nonzero()[0].tolist())}")


def test_fused_upsum_equals_the_launch_chain(pkg):
    lib = pkg._lib.load()
    cases = [(32, s) for s in SHAPES] + [(48, (2, 128, 128))]
    nets = {C: (_net(pkg, C, 5), _net(pkg, C, 5, {"HH_NO_FUSED_UPSUM": "1"})) for C in (32, 48)}
    try:
        for i, (C, shape) in enumerate(cases):
            fused, plain = nets[C]
            x = torch.from_numpy(pkg.synth.synth_images(*shape, 60 + i)).to(DEV)
            for lanes in (1, 0):
                lib.hh_set_multi_lane(fused._h, lanes)
                lib.hh_set_multi_lane(plain._h, lanes)
                a = [t.clone() for t in fused.forward_raw(x)]
                b = [t.clone() for t in plain.forward_raw(x)]
                _same(a, b, f"W{C} {shape} lanes={lanes}")
                assert all(torch.isfinite(t).all() for t in a), (C, shape)
                _same(fused.forward_raw(x), a, f"W{C} {shape} lanes={lanes} repeated")
    finally:
        for pair in nets.values():
            for net in pair:
                lib.hh_set_multi_lane(net._h, 1)


def test_fused_upsum_on_poisoned_memory(pkg):
    """NaN patterns in the workspace (HH_POISON_WS=1) and in every CU's LDS in front of every launch (HH_POISON_LDS=1): the fused
    output 0 reads only what it wrote."""
    plain = _net(pkg, 32, 6, {"HH_NO_FUSED_UPSUM": "1"})
    dirty = _net(pkg, 32, 6, {"HH_POISON_WS": "1", "HH_POISON_LDS": "1"})
    for i, shape in enumerate(((2, 128, 128), (1, 32, 64), (5, 352, 416), (1, 512, 512))):
        x = torch.from_numpy(pkg.synth.synth_images(*shape, 70 + i)).to(DEV)
        ref = [t.clone() for t in plain.forward_raw(x)]
        _same(dirty.forward_raw(x), ref, f"{shape} poisoned")
