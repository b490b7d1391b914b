"""Host half of the heatmap panels (keypoints/visualization.py, hh_heatmap_panels_u8): needs the built library, no GPU.

hh_debug_heatmap_panels_host is csrc/panel_math.h, the arithmetic of the kernels, compiled for the host.  It is held byte for byte to
tests/panels_ref.py (numpy over oracle.decode.bilinear, which tests/test_oracle_cpu.py pins to torch CPU) on the lattice of
tests/panels_helpers.py.  The planted-defect test shows that this lattice can tell: each defect named in the rule's text, planted in
the restatement one at a time, changes at least one byte of a named case.

UNPINNED: the JET table and the fx / fy resize are restatements of OpenCV read from its sources; cv2 is not installed where the fixtures
are made."""
import numpy as np
import pytest
import torch

import cv_resize
import panels_ref as pr
from panels_helpers import image_of, lattice, levels_from, nibble_lut, quantiser_sweep
from render_helpers import vis  # noqa: F401


@pytest.fixture(scope="module")
def cases():
    return {name: (img, grids) for name, img, grids in lattice()}


def _host(vis, img, grids, lut=None):
    placed, Hc, Wc = vis.figure_layout(grids, img.shape[0], img.shape[1])
    return vis.panels_host(img, placed, Hc, Wc, lut)


def test_abi_and_exports(pkg):
    lib = pkg._lib.load()
    assert lib.hh_abi_version() == 3
    for name in ("hh_heatmap_panels_u8", "hh_debug_heatmap_panels_host", "hh_unnormalize_u8", "hh_resize_u8_scaled"):
        assert hasattr(lib, name) and name in pkg._lib.exported_symbols(), name
    assert callable(pkg.keypoints.jet_lut) and callable(pkg.keypoints.plot_heatmaps)
    assert hasattr(pkg.keypoints.KeypointsResult, "plot")


def test_lattice_covers_the_issue(cases):
    kinds, shapes, Ks, unused = set(), set(), set(), False
    for name, (img, grids) in cases.items():
        shapes.add(img.shape[:2])
        for maps, nrows, pad in grids:
            assert pad == 5
            Ks.add(len(maps))
            unused |= len(maps) % nrows != 0
            for kind, src, src2, f in maps:
                kinds.add((kind, f))
    assert kinds == {(k, f) for k in range(4) for f in range(4)}
    assert shapes == {(32, 48), (64, 64), (20, 28)} and Ks == {1, 3, 17} and unused
    maps = cases["kind3_flags2"][1][0][0]
    assert np.ptp(maps[0][1]) == 0 and np.isnan(maps[1][1]).sum() == 1 and np.isposinf(maps[2][1]).any() and np.isneginf(maps[2][1]).any()
    values = np.concatenate([m[1].ravel() for m in cases["mixed_8x12_K3_r1"][1][1][0]])
    assert (values < 0).any() and (values > 1).any()


def test_bilinear_of_the_reference_is_torch_cpu(vis):
    """The maps of panels_ref come from oracle.decode.bilinear, the decode's form fma(fma(a, wx0, b wx1), wy0, fma(c, wx0, d wx1) wy1).
    Here all four kinds once more against F.interpolate itself, on planes of more than 4096 output pixels: that is where torch CPU
    (2.10) computes in this form, and every real heatmap (128 x 128 and up) lies there.  On smaller output planes torch's own result
    differs from the form in the last bit (seen here: 16 x 16 -> 64 x 64 differs, 16 x 20 -> 64 x 80 does not), so the tiny planes of
    the lattice are held to the form, not to torch."""
    f = torch.nn.functional.interpolate

    def up(x, size):
        return f(torch.from_numpy(np.ascontiguousarray(x))[None, None], size=list(size), mode="bilinear", align_corners=False)[0, 0].numpy()

    for hq, wq in ((33, 33), (24, 50)):
        H, W = 4 * hq, 4 * wq
        rng = np.random.default_rng(hq)
        q, h = rng.normal(0, 1, (hq, wq)).astype(np.float32), rng.normal(0, 1, (2 * hq, 2 * wq)).astype(np.float32)
        want = {pr.SINGLE: up(q, (H, W)), pr.NESTED: up(up(q, (2 * hq, 2 * wq)), (H, W)),
                pr.AVERAGE: up(torch.stack([torch.from_numpy(up(q, (2 * hq, 2 * wq))), torch.from_numpy(h)]).mean(dim=0).numpy(), (H, W))}
        img = np.zeros((H, W, 3), np.uint8)
        for kind, ref in want.items():
            assert np.array_equal(pr.map_values(kind, q, h, H, W), ref), kind
            # and the host form of the kernels' arithmetic, through the colour index of a clipped map
            cells = vis.panels_host(img, [(kind, q, h if kind == pr.AVERAGE else None, pr.CLIP, 0, 0)], H, W, nibble_lut())
            assert np.array_equal(levels_from(cells), pr.quantise(np.clip(ref, 0, 1))), kind


def test_host_form_equals_reference_on_the_lattice(vis, cases):
    lut = pr.jet_lut()
    for name, (img, grids) in cases.items():
        ref = pr.figure(img, grids, lut)
        got = _host(vis, img, grids)
        assert got.shape == ref.shape and np.array_equal(got, ref), (name, int((got != ref).sum()))


def test_jet_lut(vis):
    lut = vis.jet_lut()
    assert lut.dtype == np.uint8 and lut.shape == (256, 3)
    assert tuple(lut[0]) == (128, 0, 0) and tuple(lut[1]) == (132, 0, 0) and tuple(lut[255]) == (0, 0, 128)
    assert np.array_equal(lut, pr.jet_lut())
    # B,G,R: blue is full at the low end, red at the high end, green in the middle
    assert lut[32, 0] == 255 and lut[192, 2] == 255 and lut[128, 1] == 255 and lut[0, 2] == 0 and lut[255, 0] == 0


def test_quantiser_equals_numpy_cast(vis):
    """Step 3 through the host form: DIRECT maps holding the sweep, no flags, a black image and a colour table that the blend keeps
    injective, so that the colour index can be read back from the pixels."""
    v = quantiser_sweep()
    W = 64
    v = np.concatenate([v, np.zeros(-len(v) % W, np.float32)]).reshape(-1, W)
    img = np.zeros(v.shape + (3,), np.uint8)
    got = levels_from(vis.panels_host(img, [(pr.DIRECT, v, None, 0, 0, 0)], v.shape[0], W, nibble_lut()))
    want = pr.quantise(v).astype(np.int32)  # numpy's own cast
    assert np.array_equal(got, want), (v[got != want][:8], got[got != want][:8], want[got != want][:8])
    # and the rule as the text states it
    with np.errstate(invalid="ignore", over="ignore"):
        q = v * np.float32(255)
        ok = np.isfinite(q) & (q >= -2.0 ** 31) & (q < 2.0 ** 31)
        t = np.where(ok, np.trunc(np.where(ok, q, 0)), 0).astype(np.int64)
    assert np.array_equal(255 - (t & 255), want)
    for x, level in ((-1.0, 255), (-3.7, 253), (-255.0, 1), (np.nan, 0), (-np.inf, 0)):
        with np.errstate(invalid="ignore"):
            assert int(np.array([x], np.float32).astype(np.uint8)[0]) == level


# defect -> the lattice case that must show it
DEFECTS = [
    ("minus_min", "mixed_8x12_K3_r1"),      # v - mn instead of v - mx
    ("drop_nan", "kind3_flags2"),           # NaN dropped in the reduction
    ("half_up", "mixed_5x7_K1_r1"),         # round-half-up in the blend
    ("swap_lut", "mixed_8x12_K1_r1"),       # B <-> R swap of the colour table
    ("nested_as_single", "kind2_flags1"),   # NESTED computed as SINGLE from 1/4
    ("stale_last", "kind0_flags0"),         # last unused cell not zeroed
]


@pytest.mark.parametrize("defect,case", DEFECTS)
def test_planted_defect_changes_a_named_case(vis, cases, defect, case):
    img, grids = cases[case]
    lut = pr.jet_lut()
    good = pr.figure(img, grids, lut)
    assert np.array_equal(_host(vis, img, grids), good)
    bad = pr.figure(img, grids, lut, **{defect: True})
    assert bad.shape == good.shape and (bad != good).any(), defect


def test_planted_defect_in_the_fx_resize(vis, cases):
    """w / W instead of 1 / fx: on the figure of a lattice case shrunk by 0.6."""
    img, grids = cases["mixed_8x12_K3_r2"]
    fig = pr.figure(img, grids, pr.jet_lut())
    good = pr.resize_scaled(fig, 0.6, 0.6)
    bad = pr.resize_scaled(fig, 0.6, 0.6, size_ratio=True)
    assert bad.shape == good.shape and (bad != good).any()


def test_resize_scaled_restatement():
    src = image_of(79, 111, 3)
    assert pr.resize_scaled(src, 0.6, 0.6).shape == (47, 67, 3) and pr.resize_scaled(src, 0.4, 0.4).shape == (32, 44, 3)
    assert pr.scaled_size(5, 0.5) == 2 and pr.scaled_size(7, 0.5) == 4 and pr.scaled_size(3, 0.5) == 2  # halves go to the even side
    # a factor that is exactly W / w gives cv2.resize(src, (W, H)), through the 2 x 2 mean and through the taps
    for (h, w), f in (((64, 48), 0.5), ((64, 48), 0.25), ((37, 48), 2.0), ((16, 24), 1.5)):
        s = image_of(h, w, 1)
        H, W = pr.scaled_size(h, f), pr.scaled_size(w, f)
        assert H / h == f and W / w == f
        assert np.array_equal(pr.resize_scaled(s, f, f), cv_resize.resize(s, (W, H))), (h, w, f)


def test_grid_layout_is_make_grid(vis):
    for n, nrows in ((1, 1), (3, 2), (17, 2), (17, 1), (4, 2)):
        assert vis.grid_layout(n, nrows, 20, 28, 5) == pr.grid_layout(n, nrows, 20, 28, 5)
    with pytest.raises(ValueError):
        vis.figure_layout([([(0, None, None, 0)] * 3, 1, 5), ([(0, None, None, 0)] * 2, 1, 5)], 20, 28)


def test_host_form_refuses_bad_arguments(pkg, vis):
    img = image_of(20, 28, 0)
    m = np.zeros((20, 28), np.float32)
    q = np.zeros((5, 7), np.float32)
    ok = [(pr.DIRECT, m, None, 0, 0, 0)]
    assert vis.panels_host(img, ok, 20, 28).shape == (20, 28, 3)
    for placed, Hc, Wc in (([(7, m, None, 0, 0, 0)], 20, 28), ([(pr.DIRECT, m, None, 4, 0, 0)], 20, 28), ([(pr.DIRECT, m, None, 0, 1, 0)], 20, 28),
                           ([(pr.DIRECT, m, None, 0, 0, -1)], 20, 28), ([(pr.DIRECT, q, None, 0, 0, 0)], 20, 28), ([(pr.NESTED, m, None, 0, 0, 0)], 20, 28),
                           ([(pr.AVERAGE, q, None, 0, 0, 0)], 20, 28), ([], 20, 28)):
        with pytest.raises(pkg._lib.HHError):
            vis.panels_host(img, placed, Hc, Wc)
