"""CPU checks of the fused output 0 of the fusion layers (fusion_up.hip, OP_UPSUM): the multi-lane schedule stays race-free with
it and without it (HH_NO_FUSED_UPSUM=1), under the other schedule switches, and the FLOP count of the forward does not change."""
import contextlib
import os


@contextlib.contextmanager
def _env(env):
    os.environ.update(env)
    try:
        yield
    finally:
        for k in env:
            del os.environ[k]


SWITCHES = ({}, {"HH_FULL_JOIN": "1"}, {"HH_NO_FUSION_MERGE": "1"}, {"HH_FULL_JOIN": "1", "HH_NO_FUSION_MERGE": "1"})


def test_plan_checker_with_and_without_fused_upsum(pkg):
    lib = pkg._lib.load()
    for upsum in ({}, {"HH_NO_FUSED_UPSUM": "1"}):
        for sw in SWITCHES:
            env = dict(upsum, **sw)
            with _env(env):
                nets = (pkg.HigherHRNet(17, 32), pkg.HigherHRNet(17, 48), pkg.HigherHRNet(5, 32), pkg.ClassificationHRNet(32, 10))
            for net in nets:
                assert lib.hh_debug_check_plan(net._h) == 0, (env, lib.hh_last_error().decode())


def test_fused_upsum_keeps_the_flop_count(pkg):
    lib = pkg._lib.load()
    for C in (32, 48):
        fused = pkg.HigherHRNet(17, C)
        with _env({"HH_NO_FUSED_UPSUM": "1"}):
            plain = pkg.HigherHRNet(17, C)
        for B, H, W in ((32, 512, 512), (1, 32, 64), (5, 352, 416)):
            a = lib.hh_forward_flops(fused._h, B, H, W)
            b = lib.hh_forward_flops(plain._h, B, H, W)
            assert a == b and a > 0, (C, B, H, W, a, b)
