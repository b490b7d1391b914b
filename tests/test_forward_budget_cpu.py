"""The error budgets of tests/forward_budget.py and the host-side tile walk of the fused 32-channel block, without a GPU."""
import ctypes

import numpy as np
import pytest
import torch

import forward_budget as fb
from oracle import forward as ofw


def _old_close_passes(got, ref) -> bool:
    """what test_gpu_parity._close asserts: the two global figures against TOL_MAX / TOL_RMS"""
    f = fb.figures(got, ref)
    return f["max"][0] <= fb.TOL_MAX and f["rms"][0] <= fb.TOL_RMS


def test_storage_argument_of_the_oracle():
    """storage="fp32" is the default path (the goldens of test_oracle_cpu.py pin that one bit for bit); bf16 is another result, with
    bf16 values where the rule rounds; anything else, or bf16 with batch-statistics BatchNorm, is refused."""
    sd, x = fb.state_dict(32, 0), fb.images((1, 64, 64), 0)
    with torch.no_grad():
        a, at = ofw.higher_hrnet(x, sd, 17)
        b, bt = ofw.higher_hrnet(x, sd, 17, storage="fp32")
        hms, tags, taps = ofw.higher_hrnet(x, sd, 17, return_taps=True, storage="bf16")
        c, ct = ofw.higher_hrnet(x, sd, 17)  # the switch does not stick
    assert all(torch.equal(u, v) for u, v in zip(a + [at], b + [bt])) and all(torch.equal(u, v) for u, v in zip(a + [at], c + [ct]))
    assert not torch.equal(hms[1], a[1])
    for name in ("stem#0", "stages.1#0", "stages.3.blocks.5#0", "deconv#0", "deconv#1"):
        t = taps[name]
        assert torch.equal(t, t.to(torch.bfloat16).to(torch.float32)), name
    with pytest.raises(ValueError):
        ofw.higher_hrnet(x, sd, 17, storage="fp16")
    with pytest.raises(ValueError):
        ofw.higher_hrnet(x, sd, 17, train=True, storage="bf16")
    with pytest.raises(ValueError):
        ofw.classification_hrnet(x, sd, storage="half")


@pytest.mark.parametrize("shape,seed", [((1, 64, 64), 0), ((2, 128, 128), 1), ((4, 32, 32), 2)])
def test_emulation_stays_inside_the_stated_tolerance(shape, seed):
    """The caps of the budgets (TOL_MAX / TOL_RMS) never bind on the reference alone: the bf16-storage emulation meets them at every
    tap and output, and every budget is a positive number."""
    ref, emu = fb.tensors(shape, 32, seed)
    assert len(ref) >= 60
    worst = {"max": 0.0, "rms": 0.0}
    for name in ref:
        f = fb.figures(emu[name], ref[name])
        assert f["max"][0] <= fb.TOL_MAX and f["rms"][0] <= fb.TOL_RMS, (name, f)
        assert all(v > 0 for v in fb.allowed(f).values()), name
        fb.check(emu[name], ref[name], fb.allowed(f), name)  # (and the emulation passes its own budget)
        worst = {k: max(worst[k], f[k][0]) for k in worst}
    print(f"{shape}: emulation worst max {worst['max']:.4f} rms {worst['rms']:.4f}")


def test_classifier_emulation_stays_inside_the_stated_tolerance():
    ref, emu = fb.tensors((2, 64, 96), 32, 11, None, True)
    f = fb.figures(emu["logits"], ref["logits"])
    assert f["max"][0] <= fb.TOL_MAX and f["rms"][0] <= fb.TOL_RMS, f
    assert np.array_equal(emu["logits"].argmax(1), ref["logits"].argmax(1))


def _fails(got, ref, emu, what):
    with pytest.raises(AssertionError) as e:
        fb.check(got, ref, fb.allowed(fb.figures(emu, ref)), what)
    return str(e.value)


def test_check_catches_planted_defects():
    """Defects of the kind a tiling bug makes, planted on the emulated tensors and compared with the fp32 oracle under the emulation's
    own budget: check() must fail each, and name the place.  All four are caught at the sizes first chosen (10 % column, 3 % image: no
    bisection towards larger defects was needed).  OLD records what test_gpu_parity._close (global max 5e-2, rms 2e-2) says of the same tensors: it lets a last
    column that is 10 % low through on hm_h and one image of eight that is 3 % low on every tensor."""
    OLD = {}  # (defect, tensor) -> does the old global check pass the defective tensor?
    ref, emu = fb.tensors((2, 128, 128), 32, 1)
    for name in ("hm_h", "hm_q", "stem#0"):
        r, e = ref[name], emu[name]
        g = e.copy()
        g[-1, :, -1, :] = g[-1, :, -2, :]  # one border row of the last image replaced by its neighbour
        msg = _fails(g, r, e, name)
        assert f"image 1 row {r.shape[2] - 1}" in msg, msg
        OLD["row", name] = _old_close_passes(g, r)
        g = e.copy()
        g[0, :, :, -1] *= 0.9  # the last column of image 0, 10 % low
        msg = _fails(g, r, e, name)
        assert f"image 0 column {r.shape[3] - 1}" in msg, msg
        OLD["col", name] = _old_close_passes(g, r)
    ref, emu = fb.tensors((8, 64, 96), 32, 2)
    for name in ("hm_h", "hm_q", "stem#0"):
        r, e = ref[name], emu[name]
        g = e.copy()
        g[5] *= 0.97  # one image of eight, 3 % low
        msg = _fails(g, r, e, name)
        assert "img" in msg and "image 5" in msg, msg
        OLD["img", name] = _old_close_passes(g, r)
    # two rows of one image of a 32 x 17 x 8 x 8 map keep what the workspace held: the rows of another forward
    ref, emu = fb.tensors((32, 32, 32), 32, 3)
    stale = fb.tensors((32, 32, 32), 32, 3, 7)[1]
    r, e = ref["hm_q"], emu["hm_q"]
    assert r.shape == (32, 17, 8, 8)
    g = e.copy()
    g[11, :, 0:2, :] = stale["hm_q"][11, :, 0:2, :]
    msg = _fails(g, r, e, "hm_q")
    assert "image 11 row" in msg, msg
    OLD["stale", "hm_q"] = _old_close_passes(g, r)
    g = e.copy()
    g[11, :, 0:2, :] = np.nan  # and under HH_POISON_WS the unwritten rows are NaN: an infinite error, never a skipped value
    assert "image 11 row 0" in _fails(g, r, e, "hm_q")
    assert OLD == {("row", "hm_h"): False, ("row", "hm_q"): False, ("row", "stem#0"): False,
                   ("col", "hm_h"): True, ("col", "hm_q"): False, ("col", "stem#0"): False,
                   ("img", "hm_h"): True, ("img", "hm_q"): True, ("img", "stem#0"): True,
                   ("stale", "hm_q"): False}, OLD


def test_budget_is_never_looser_than_the_stated_tolerance():
    b = fb.allowed({k: (1.0, "") for k in fb.FIGURES})
    assert b["max"] == fb.TOL_MAX and b["rms"] == fb.TOL_RMS
    b = fb.budget("stem#0", (1, 64, 64), 32, 0)
    assert b["max"] < 0.02 and b["rms"] < 0.01, b  # the stem's budget: a fraction of the global tolerance


def test_fused_block_tiles_cover_every_row_exactly_once(pkg):
    """hh_debug_bb_cover walks every tile of the launch bbpc_launch would make through the kernel's own row arithmetic: every output
    row stored exactly once, every input / intermediate row a stored row needs present in its tile, for every shape the launcher
    takes.  (Before the H + 2 > TH guard of the tall layout this sweep failed in 2227 of its 32670 cases, all at map heights of 9
    rows and less: e.g. 32 x 8 x 8, tall = 1: 8 row segments never stored -- rows 0, 1 of images 4, 11, 18, 25.)"""
    lib = pkg._lib.load()
    c = (ctypes.c_int64 * 4)()
    n, bad = 0, []
    for B in range(1, 34):
        for H in list(range(1, 65)) + [128, 256]:
            for W in (8, 32, 40, 64, 128):
                for tall in (0, 1, 2):
                    for cus in (256,) if (B + H) % 4 else (256, 7):  # (a grid smaller than the tile count: the strided tile walk)
                        pkg._lib.check(lib.hh_debug_bb_cover(B, H, W, tall, cus, c))
                        n += 1
                        if any(c):
                            bad.append((B, H, W, tall, cus, list(c)))
    assert n >= 32670
    assert not bad, f"{len(bad)} of {n} cases; unstored / stored twice / lost input rows / lost mid rows: {bad[:8]}"
    assert lib.hh_debug_bb_cover(0, 8, 8, 1, 256, c) != 0 and lib.hh_debug_bb_cover(1, 8, 8, 3, 256, c) != 0
