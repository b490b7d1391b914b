"""The budgets of tests/train_budget.py hold what they should, without a GPU: a CPU emulation of the kernels' arithmetic (torch fp32 on
the same operands, bf16 where the kernel stores bf16) stays inside every budget on every lattice case, every planted defect of the
emulation is flagged where it sits, and the lattice reaches the kernel instantiations, tile-width fallbacks and weight-gradient
variants it claims to (asked of the library's own selection code: hh_conv2d_config, hh_conv2d_wgrad_plan)."""
import ctypes
import re

import pytest
import torch

import train_budget as tb

CONV = {tb.conv_id(c): c for c in tb.CONV_CASES}


def _flags(fn, *needles, border=None, interior=None):
    """fn must fail in tb.check; its message must hold every needle, and its counts of offenders on the border (first / last row or
    column, last image) and in the interior must be as stated: ">0", or a number.  (check() names both parts in every message, so
    only the counts say where a defect sits.)"""
    with pytest.raises(AssertionError) as e:
        fn()
    msg = str(e.value)
    for n in needles:
        assert n in msg, (n, msg)
    for part, want in (("border", border), ("interior", interior)):
        got = int(re.search(part + r" (\d+)", msg).group(1))
        if want is not None:
            assert (got > 0) if want == ">0" else (got == want), (part, want, msg)
    return msg


# ------------------------------------------------------------------------------------------------ the budgets are not too tight
@pytest.mark.parametrize("case", tb.CONV_CASES, ids=tb.conv_id)
def test_conv_emulation_within_budget(case):
    refs, emu = tb.conv_refs(case), tb.emulate_conv(tb.conv_inputs(case), case)
    worst = {k: tb.check(emu[k], *refs[k], f"{tb.conv_id(case)} {k}") for k in ("fwd", "dgrad", "dgrad_res")}
    ref, hard, sens = refs["wgrad"]
    worst["wgrad hard"] = tb.check(emu["wgrad"], ref, hard, f"{tb.conv_id(case)} wgrad (hard bound)", spatial=False)
    worst["wgrad sensitive"] = tb.check(emu["wgrad"], ref, sens, f"{tb.conv_id(case)} wgrad (sensitive bound)", spatial=False)
    print("emulation / allowed", tb.conv_id(case), {k: round(v, 3) for k, v in worst.items()})


@pytest.mark.parametrize("case", tb.BN_CASES, ids=tb.bn_id)
def test_bn_emulation_within_budget(case):
    i = tb.bn_inputs(case)
    fw = tb.emulate_bn_forward(i, case)
    worst = {k: tb.check(fw[k], *v, f"{tb.bn_id(case)} {k}", spatial=k == "y") for k, v in tb.bn_forward_refs(case).items()}
    bw = tb.emulate_bn_backward(i, case, fw)
    for k, v in tb.bn_backward_refs(case, fw["y"]).items():
        worst[k] = tb.check(bw[k], *v, f"{tb.bn_id(case)} {k}", spatial=k in ("dx", "dres"))
    print("emulation / allowed", tb.bn_id(case), {k: round(v, 3) for k, v in worst.items()})


@pytest.mark.parametrize("case", tb.FUSION_CASES, ids=tb.fusion_id)
def test_fusion_emulation_within_budget(case):
    i = tb.fusion_inputs(case)
    out = tb.emulate_fusion(i, case)
    worst = [tb.check(out, *tb.fusion_forward_ref(case), f"{tb.fusion_id(case)} out")]
    for j, (g, r) in enumerate(zip(tb.emulate_fusion_backward(i, case, out), tb.fusion_backward_refs(case, out))):
        worst.append(tb.check(g, *r, f"{tb.fusion_id(case)} gradient of term {j}"))
    print("emulation / allowed", tb.fusion_id(case), [round(v, 3) for v in worst])


# ------------------------------------------------------------------------------------------------ the budgets are not too loose
def test_check_reports_nan_border_and_interior():
    ref = torch.zeros(2, 3, 5, 6, dtype=torch.float64)
    allowed = torch.full_like(ref, 1e-3)
    assert tb.check(ref + 5e-4, ref, allowed, "x") == pytest.approx(0.5)
    got = ref.clone()
    got[0, 1, 2, 3] = float("nan")
    _flags(lambda: tb.check(got, ref, allowed, "x"), "1 of 180", "border 0", "interior 1 in [0, 1, 2, 3] .. [0, 1, 2, 3]", "inf x allowed")
    got = ref.clone()
    got[1, 0, 2, 2] = got[0, 0, 4, 1] = got[0, 2, 1, 0] = 1.0
    _flags(lambda: tb.check(got, ref, allowed, "x"), "3 of 180", "border 3 in [0, 0, 1, 0] .. [1, 2, 4, 2]", "interior 0")
    assert tb.check(ref, ref, torch.zeros_like(ref), "x") == 0.0
    _flags(lambda: tb.check(ref[0, 0] + 1e-9, ref[0, 0], torch.zeros(5, 6), "x", spatial=False), "30 of 30", "interior 30")


def test_planted_conv_forward_defects_are_flagged():
    c = CONV["64to64-k3s1-3x16x24-p11"]
    i, (ref, allowed) = tb.conv_inputs(c), tb.conv_refs(c)["fwd"]
    # one (tap, channel) term dropped
    j = dict(i, w=i["w"].clone())
    j["w"][:, 17, 0, 2] = 0
    msg = _flags(lambda: tb.check(tb.bf(tb.conv_forward(j, c)), ref, allowed, "term dropped"), border=">0", interior=">0")
    assert int(msg.split(": ")[1].split(" of")[0]) > 0.3 * ref.numel(), msg  # (ReLU zeroes some; the issue's 49-84 % are before it)
    # last output row missing one kernel row
    got = tb.bf(tb.conv_forward(i, c))
    j = dict(i, w=i["w"].clone())
    j["w"][:, :, 0, :] = 0
    got[:, :, -1] = tb.bf(tb.conv_forward(j, c))[:, :, -1]
    _flags(lambda: tb.check(got, ref, allowed, "last row"), f"[0, 0, {c.H - 1}, 0] ..", border=">0", interior=0)
    # the last column tile (columns >= 32 of a 40-wide map) zero
    c = CONV["48to48-k3s1-3x24x40-p11"]
    i, (ref, allowed) = tb.conv_inputs(c), tb.conv_refs(c)["fwd"]
    got = tb.bf(tb.conv_forward(i, c))
    got[..., 32:] = 0
    msg = _flags(lambda: tb.check(got, ref, allowed, "last tile"), border=">0", interior=">0")
    assert ", 32] .. [" in msg.split("interior")[1], msg  # the interior offenders start at column 32


def test_planted_data_gradient_defects_are_flagged():
    c = CONV["64to64-k3s1-3x16x24-p11"]
    i, refs = tb.conv_inputs(c), tb.conv_refs(c)
    for name, w in (("kernel not rotated", i["w"].flip(2, 3)), ("ky / kx transposed", i["w"].transpose(2, 3))):
        got = tb.bf(tb.conv_grads(i["x"], w, i["dy"], c)[0])
        _flags(lambda: tb.check(got, *refs["dgrad"], name), interior=">0")
    got = tb.emulate_conv(i, c)["dgrad"]  # res not added
    _flags(lambda: tb.check(got, *refs["dgrad_res"], "res not added"), interior=">0")
    # 2x2: pad not flipped = the data gradient of the conv with the other padding
    for cid in ("80to32-k2s1-3x6x40-p00", "80to32-k2s1-3x3x17-p01", "80to32-k2s1-1x17x24-p10", "80to32-k2s1-3x2x12-p11"):
        c = CONV[cid]
        i = tb.conv_inputs(c)
        got = tb.emulate_conv(i, c, pad_dgrad=(1 - c.pad[0], 1 - c.pad[1]))["dgrad"]
        # an interior needs an image that is not the last, a row and a column that are neither first nor last
        inside = c.B > 1 and c.H > 2
        _flags(lambda: tb.check(got, *tb.conv_refs(c)["dgrad"], "pad not flipped " + cid), border=">0", interior=">0" if inside else 0)
    # stride 2: phase (1, 0) taken from phase (0, 1)
    c = CONV["48to96-k3s2-3x12x48-p11"]
    got = tb.emulate_conv(tb.conv_inputs(c), c)["dgrad"].clone()
    got[:, :, 1::2, 0::2] = got[:, :, 0::2, 1::2]
    _flags(lambda: tb.check(got, *tb.conv_refs(c)["dgrad"], "phase swapped"), interior=">0")


def test_planted_weight_gradient_defects_are_flagged():
    # one 4 x 32 tile of one image dropped at n = 65536: inside the hard bound, outside the sensitive one
    c = tb.WGRAD_N65536
    i = tb.conv_inputs(c)
    ref, hard, sens = tb.conv_refs(c)["wgrad"]
    dy = i["dy"].clone()
    dy[2, :, 64:68, 32:64] = 0
    got = tb.conv_grads(i["x"], i["w"], dy, c)[1]
    assert tb.check(got, ref, hard, "tile dropped, hard bound", spatial=False) < 1
    _flags(lambda: tb.check(got, ref, sens, "tile dropped, sensitive bound", spatial=False), border=0, interior=">0")
    # the last H % 4 rows dropped
    c = CONV["48to96-k3s1-3x6x40-p11"]
    i = tb.conv_inputs(c)
    ref, hard, sens = tb.conv_refs(c)["wgrad"]
    dy = i["dy"].clone()
    dy[:, :, 4:] = 0
    got = tb.conv_grads(i["x"], i["w"], dy, c)[1]
    _flags(lambda: tb.check(got, ref, sens, "last rows dropped", spatial=False), border=0, interior=">0")
    # ks = 2: pad off by one
    for cid in ("80to32-k2s1-3x6x40-p00", "80to32-k2s1-3x3x17-p01", "80to32-k2s1-1x17x24-p10", "80to32-k2s1-3x2x12-p11"):
        c = CONV[cid]
        got = tb.emulate_conv(tb.conv_inputs(c), c, pad_wgrad=(c.pad[0], 1 - c.pad[1]))["wgrad"]
        _flags(lambda: tb.check(got, *tb.conv_refs(c)["wgrad"][:2], "pad off by one " + cid, spatial=False), border=0, interior=">0")


def test_planted_batchnorm_defects_are_flagged():
    by_id = {tb.bn_id(c): c for c in tb.BN_CASES}
    c = by_id["C32-1x97x1-res-special"]  # P = 97: 1 / (P - 1) is 1 % off 1 / P
    i, fr = tb.bn_inputs(c), tb.bn_forward_refs(c)
    fw = tb.emulate_bn_forward(i, c, unbiased=True)
    _flags(lambda: tb.check(fw["invstd"], *fr["invstd"], "unbiased variance", spatial=False), border=0, interior=">0")
    fw = tb.emulate_bn_forward(i, c)
    br = tb.bn_backward_refs(c, fw["y"])
    # (a 1 x 97 x 1 map: one image, one column, so every element is on the border)
    _flags(lambda: tb.check(tb.emulate_bn_backward(i, c, fw, dbeta_pm1=True)["dx"], *br["dx"], "dbeta / (P - 1)"), border=">0", interior=0)
    c = by_id["C32-3x24x24-relu-special"]
    i, fr = tb.bn_inputs(c), tb.bn_forward_refs(c)
    fw = tb.emulate_bn_forward(i, c)
    br = tb.bn_backward_refs(c, fw["y"])
    _flags(lambda: tb.check(tb.emulate_bn_backward(i, c, fw, no_mask=True)["dx"], *br["dx"], "ReLU mask ignored"), interior=">0")
    _flags(lambda: tb.check(tb.emulate_bn_backward(i, c, fw, no_dgamma_term=True)["dx"], *br["dx"], "dx without the dgamma term"), interior=">0")
    # the zero pre-activation channel: y is exactly 0 there, so those pixels carry no gradient
    assert (fw["y"][:, 2] == 0).sum() >= c.B * c.H * c.W // 3 and (tb.bn_backward_refs(c, fw["y"])["dbeta"][0][2] != tb.bn_inputs(c)["dy"][:, 2].double().sum())
    # The clamp.  In the kernels' double arithmetic b / P - m^2 of a constant channel is exactly 0 and the clamp is idle; it guards sums
    # that round.  So the defect is planted where it bites: the same sums in fp32, where b / P - m^2 of the constant channel (100.5,
    # P = 1728) comes out at -0.19.  With the clamp that is 0 and invstd = 1 / sqrt(eps) sits inside the budget; without it invstd is a NaN.
    const = [r[1:2] for r in fr["invstd"]]
    assert abs(float(const[0]) - tb.BN_EPS ** -0.5) < 1e-9
    assert tb.check(tb.emulate_bn_forward(i, c, fp32_var="clamped")["invstd"][1:2], *const, "constant channel: fp32 variance, clamped", spatial=False) < 1
    bad = tb.emulate_bn_forward(i, c, fp32_var="unclamped")["invstd"][1:2]
    assert bad.isnan().all()
    _flags(lambda: tb.check(bad, *const, "constant channel: fp32 variance, not clamped", spatial=False), "inf x allowed", border=0, interior=1)


def test_planted_fusion_defects_are_flagged():
    by_id = {tb.fusion_id(c): c for c in tb.FUSION_CASES}
    c = by_id["C32-3x32x64-s0125-relu"]
    i = tb.fusion_inputs(c)
    _flags(lambda: tb.check(tb.emulate_fusion(i, c, offset=1), *tb.fusion_forward_ref(c), "nearest index (y + 1) >> s"), interior=">0")
    out = tb.emulate_fusion(i, c)
    grads, refs = tb.emulate_fusion_backward(i, c, out), tb.fusion_backward_refs(c, out)
    g = i["dy"] * (out > 0)
    # the shift-5 term's gradient at [1, 7, 0, 1] without the last of its 1024 addends (one that the mask kept)
    blk = g[1, 7, 0:32, 32:64]
    last = blk.flatten()[blk.flatten().nonzero()[-1, 0]]
    bad = grads[3].clone()
    bad[1, 7, 0, 1] = tb.bf(blk.sum() - last)
    _flags(lambda: tb.check(bad, *refs[3], "one addend missing"), "worst at [1, 7, 0, 1]", border=1, interior=0)  # row 0 of a 1 x 2 map


# ------------------------------------------------------------------------------------------------ what the lattice reaches
def _cfg(lib, i):
    out = (ctypes.c_int * 7)()
    assert lib.hh_conv_config(i, out) == 0
    return dict(zip(("KS", "S", "KC", "NT", "WC", "PT", "TW"), out))


def _run_config(lib, c, mode):
    """(instantiation, Wo) of the case's forward (mode 0) or data gradient (mode 1 / 2)"""
    Wo = c.W // 2 if c.stride == 2 else c.W  # what the launched conv writes: in mode 2 the W of dL/dy, per phase
    return lib.hh_conv2d_config(c.cin, c.cout, c.ks, c.stride, mode, Wo), Wo


def test_lattice_reaches_every_instantiation_fallback_and_wgrad_variant(pkg):
    lib = pkg._lib.load()
    ncfg = next(i for i in range(64) if lib.hh_conv_config(i, (ctypes.c_int * 7)()) != 0)
    db0 = {i for i in range(ncfg) if lib.hh_conv_config_double_buffered(i) == 0}
    assert len(db0) == 17
    # what each mode can reach at all: every accepted (cin, cout, ks, stride) up to 512 channels on a narrow and a wide map
    reach = {0: set(), 1: set(), 2: set()}
    chans = range(8, 513, 8)
    for mode in reach:
        for ks, stride in ((1, 1), (2, 1), (3, 1), (3, 2)):
            for cin in chans:
                for cout in chans:
                    for Wo in (8, 40):
                        reach[mode].add(lib.hh_conv2d_config(cin, cout, ks, stride, mode, Wo))
        reach[mode].discard(-1)
    assert reach[0] == db0 and reach[2] == {15, 16}, reach
    assert lib.hh_conv2d_config(3, 64, 3, 2, 0, 32) == -1 and lib.hh_conv2d_config(64, 64, 3, 2, 1, 32) == -1  # refused like the launch refuses
    seen = {0: set(), 1: set(), 2: set()}
    fallbacks = set()
    for c in tb.CONV_CASES:
        for mode in (0, 2 if c.stride == 2 else 1):
            cfg, Wo = _run_config(lib, c, mode)
            assert cfg >= 0, (tb.conv_id(c), mode)
            seen[mode].add(cfg)
            if (_cfg(lib, cfg)["TW"] == 16) != (Wo <= 16):
                k = _cfg(lib, cfg)
                fallbacks.add((k["KS"], k["S"], k["KC"], k["NT"], "narrow map" if Wo <= 16 else "wide map"))
    for mode in seen:
        assert seen[mode] == reach[mode], f"mode {mode}: the lattice misses instantiations {sorted(reach[mode] - seen[mode])}"
    # every (family, map width) without an instantiation of its own width, from the table itself
    fams = {}
    for i in db0:
        k = _cfg(lib, i)
        fams.setdefault((k["KS"], k["S"], k["KC"], k["NT"]), set()).add(k["TW"])
    want = {f + ("narrow map" if 16 not in tws else "wide map",) for f, tws in fams.items() if len(tws) == 1}
    assert len(want) == 7 and fallbacks == want, (sorted(want - fallbacks), sorted(fallbacks - want))
    # weight gradient: all six variants, each with one case of one tile per worker and one of more tiles than workers, unevenly split
    single, uneven = set(), set()
    out = (ctypes.c_int * 3)()
    for c in tb.CONV_CASES:
        assert lib.hh_conv2d_wgrad_plan(c.B, c.H, c.W, c.cin, c.cout, c.ks, c.stride, out) == 0
        variant, workers, tiles = out
        assert 0 <= variant <= 5 and 1 <= workers <= tiles
        if tiles == workers:
            single.add(variant)
        elif tiles % workers:
            uneven.add(variant)
    assert single == uneven == set(range(6)), (single, uneven)
    assert lib.hh_conv2d_wgrad_plan(1, 8, 8, 12, 16, 3, 1, out) == 1 and lib.hh_conv2d_wgrad_plan(1, 8, 8, 16, 16, 2, 2, out) == 1
    print(f"forward instantiations {sorted(seen[0])}; data gradient mode 1 {sorted(seen[1])}, mode 2 {sorted(seen[2])}; fallbacks {sorted(fallbacks)}; "
          f"weight-gradient variants with one tile per worker {sorted(single)}, with an uneven split {sorted(uneven)}")


def test_lattice_covers_the_listed_shapes():
    cs = tb.CONV_CASES
    maps = [tb.conv_out_hw(c) for c in cs] + [(c.H, c.W) for c in cs]
    assert {2, 3, 6, 1} <= {h for h, _ in maps} and {12, 16, 17, 24, 40} <= {w for _, w in maps}
    assert any(h > w for h, w in maps) and any(w > h for h, w in maps) and {1, 3, 5} <= {c.B for c in cs}
    pairs = {(c.cin, c.cout, c.ks, c.stride) for c in cs}
    assert {(16, 64, 3, 2), (48, 96, 3, 2), (96, 192, 3, 2), (192, 384, 3, 2), (32, 48, 1, 1), (48, 32, 1, 1), (80, 32, 2, 1), (96, 48, 2, 1)} <= pairs
    assert {c.pad for c in cs if c.ks == 2} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert any(c.B * h * w == 65536 for c, (h, w) in zip(cs, maps))
    bn = tb.BN_CASES
    assert {c.C for c in bn} == {8, 16, 32, 48, 64, 96, 192, 256, 384, 2048} and {2, 97, 1728} <= {c.B * c.H * c.W for c in bn}
    assert any(c.C == 32 and c.B * c.H * c.W > 49152 for c in bn) and any(c.B * c.H * c.W * c.C / 8 / 256 > 8192 for c in bn)
    assert {(c.res, c.relu) for c in bn} == {(a, b) for a in (False, True) for b in (False, True)} and any(c.special for c in bn)
    fu = tb.FUSION_CASES
    assert {c.C for c in fu} == {8, 32, 48, 128} and {len(c.shifts) for c in fu} == {1, 2, 3, 4} and max(max(c.shifts) for c in fu) == 5
    assert {c.relu for c in fu} == {False, True} and any(c.B % 2 for c in fu)
