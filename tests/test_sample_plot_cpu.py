"""Host half of the dataset sample figures (keypoints/sample_plot.py, hh_seg_overlay_u8_batch): no GPU needed.

The overlay's rule is restated in tests/seg_overlay_ref.py; hh_debug_seg_overlay_host (the kernel's tile walk compiled for the host) must
equal it byte for byte.  The golden (tests/golden/sample_plot.npz, tools/make_sample_plot_golden.py) was produced by the reference's own
plot_raw / plot / plot_examples over a stub dataset with recording stand-ins for cv2 and albumentations: parity of the rasterised
boundary pixels with cv2 and of the letterbox with albumentations is UNPINNED (include/hhrnet.h, keypoints/sample_plot.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import seg_overlay_ref as sr
from conftest import GOLDEN, REPO
from sample_plot_helpers import obj, overlay_cases, reference, rle_obj, sample_golden, sp  # noqa: F401


def test_abi_and_exports(pkg, sp):
    lib = pkg._lib.load()
    assert lib.hh_abi_version() == 3
    for name in ("hh_seg_overlay_u8_batch", "hh_seg_overlay_config", "hh_debug_seg_overlay_host"):
        assert hasattr(lib, name) and name in pkg._lib.exported_symbols(), name
    Th, Tw, threads, chunk = sp.overlay_config()
    assert Th >= 1 and Tw >= 1 and threads % 64 == 0 and chunk >= 1
    assert sp.DESC is pkg._lib.struct_dtype("hh_render_desc") and "hh_seg_desc" not in pkg._lib.parse_structs(open(pkg._lib.HEADER).read())


def test_cases_cover_the_issue(sp):
    Th, Tw, _, chunk = sp.overlay_config()
    cases = {c[0]: c for c in overlay_cases(sp)}
    sizes = {c[1].shape[:2] for c in cases.values()}
    assert {(1, 1), (45, 300), (64, 37)} <= sizes and 45 > Th and 300 > 2 * Tw and 64 > Th and 37 < Tw
    assert len(cases["no_shapes"][2]) == 0 and len(cases["chunks"][2]) > chunk
    assert any(c[5] for c in cases.values()) and (cases["outside"][2][:, 2:6] < 0).any()
    rle = cases["rle"][2]
    assert rle[-1, 0] == sr.FILL and (rle[:, 0] == sr.FILL).sum() == 2  # the run-length object: a fill and no contour
    # an empty fill (a polygon wholly outside) stays a row, so that the table keeps the reference's order
    assert ((cases["outside"][2][:, 0] == sr.FILL) & (cases["outside"][2][:, 3] == 0)).any()


def test_host_twin_equals_numpy_reference(sp):
    for case in overlay_cases(sp):
        name, image, shapes, toggles, alpha, bgr = case
        want = reference(case)
        assert np.array_equal(sp.overlay_host(image, shapes, toggles, alpha, bgr), want), name
        assert np.array_equal(sp.overlay_host(image, shapes, toggles, alpha, bgr, in_place=True), want), name + " (in place)"
    # an uncovered pixel is rintf(p * w0 + p * w1), not p: addWeighted's behaviour
    p = np.arange(256, dtype=np.uint8).reshape(16, 16, 1).repeat(3, 2)
    blended = sp.overlay_host(p, np.zeros((0, 8), np.int32), np.zeros(0, np.uint32), 0.4)
    assert np.array_equal(blended, sr.blend(p, p, np.float32(0.6), np.float32(0.4)))
    print(f"uncovered pixels that the blend changes at alpha 0.4: {int((blended != p).any(-1).sum())} of 256 grey levels")


def test_last_row_wins(sp):
    """Three overlapping objects: where all three cover a pixel it has the third one's colour."""
    name, image, shapes, toggles, alpha, _ = next(c for c in overlay_cases(sp) if c[0] == "last_wins")
    h, w = image.shape[:2]
    out = sp.overlay_host(image, shapes, toggles, 1.0)  # alpha 1: the overlay itself
    masks = {}
    for row in shapes:
        masks.setdefault(int(row[1]), np.zeros((h, w), bool))
        masks[int(row[1])] |= sr.shape_mask(row, toggles, h, w)
    colours = list(masks)
    assert len(colours) == 3
    all_three = masks[colours[0]] & masks[colours[1]] & masks[colours[2]]
    assert all_three.sum() > 50
    last = colours[2]
    assert (out[all_three] == (last & 255, last >> 8 & 255, last >> 16 & 255)).all()


LINES = [(2, 3, 17, 3), (5, 1, 5, 19), (0, 0, 12, 12), (12, 0, 0, 12), (0, 0, 4, 2), (0, 0, 2, 4), (0, 0, 4, -2), (0, 0, -2, 4), (3, 7, 3, 7),
         (0, 0, 10, 5), (0, 0, 10, 3), (-7, -9, 13, 4), (1, 1, 2, 30), (0, 0, 7, 7), (0, 5, 6, 2), (100, -50, -3, 17), (0, 0, 1, 0), (0, 0, 6, 3)]


def test_line_rule_against_the_nearest_pixel_walk():
    """A test of the numpy REFERENCE (tests/seg_overlay_ref.py), not of the library: the stated rule draws, along the major axis, the
    nearest pixel of the minor one, an exact tie toward plus infinity after the ends were put in order; a line and its reverse therefore
    draw the same pixels, ties included.  The library's line code is held against this reference by
    test_host_twin_lines_equal_the_rule and, on the device, by tests/test_gpu_sample_plot.py."""
    ties = 0
    rng = np.random.default_rng(5)
    for xa, ya, xb, yb in LINES + [tuple(int(v) for v in rng.integers(-40, 40, 4)) for _ in range(300)]:
        want, t = sr.nearest_walk(xa, ya, xb, yb)
        ties += t
        assert sorted(sr.line_pixels(xa, ya, xb, yb)) == sorted(want), (xa, ya, xb, yb)
        assert sorted(sr.line_pixels(xb, yb, xa, ya)) == sorted(want), ("reversed", xa, ya, xb, yb)
    assert ties > 50
    # the tie rule as stated: (0,0) -> (4,2) passes (1, 0.5) and (3, 1.5): both go up, from either end
    assert sr.line_pixels(0, 0, 4, 2) == [(0, 0), (1, 1), (2, 1), (3, 2), (4, 2)] == sr.line_pixels(4, 2, 0, 0)
    assert sr.line_pixels(0, 0, 4, -2) == [(0, 0), (1, 0), (2, -1), (3, -1), (4, -2)]
    assert sr.line_pixels(0, 0, 2, 4) == [(0, 0), (1, 1), (1, 2), (2, 3), (2, 4)]


def test_host_twin_lines_equal_the_rule(sp):
    """Every line of the list, and its reverse, shifted over a frame that spans several tiles: the column-wise solution of the kernel
    (one run of rows per column) against the rule walked along the major axis."""
    Th, Tw, _, _ = sp.overlay_config()
    h, w = Th + 9, Tw + 11
    image = np.zeros((h, w, 3), np.uint8)
    rng = np.random.default_rng(6)
    lines = LINES + [tuple(int(v) for v in rng.integers(-30, 200, 4)) for _ in range(200)]
    for n, (xa, ya, xb, yb) in enumerate(lines):
        ox, oy = (Tw - 6, Th - 6) if n % 2 else (0, 0)
        for ends in ((xa + ox, ya + oy, xb + ox, yb + oy), (xb + ox, yb + oy, xa + ox, ya + oy)):
            row = np.array([[sr.LINE, 0xFFFFFF, *ends, 0, 0]], np.int32)
            got = sp.overlay_host(image, row, np.zeros(0, np.uint32), 1.0)[..., 0] == 255
            assert np.array_equal(got, sr.line_mask(*ends, h, w)), ends


def _polygon_cover(sp, poly, h, w, shift):
    shapes, toggles = sp.seg_tables([obj(poly)], h, w, shift=shift)
    return sr.covered(shapes, toggles, h, w)


def test_fill_and_contour_leave_no_seam(sp):
    """300 seeded star-shaped integer polygons: every pixel whose integer point lies strictly inside the polygon is covered by fill or
    contour.  The same polygons filled WITHOUT the +0.5 shift violate it (the fill then stops a pixel short of right and bottom slanted
    edges), so the property can fail."""
    rng = np.random.default_rng(300)
    missed = missed_unshifted = inside_total = 0
    for _ in range(300):
        h, w = int(rng.integers(20, 91)), int(rng.integers(20, 121))
        poly = sr.star_polygon(rng, h, w)
        inside = sr.strictly_inside(poly, h, w)
        inside_total += int(inside.sum())
        missed += int((inside & ~_polygon_cover(sp, poly, h, w, 0.5)).sum())
        missed_unshifted += int((inside & ~_polygon_cover(sp, poly, h, w, 0.0)).sum())
    print(f"strictly inside: {inside_total} pixels; uncovered with the shift: {missed}; without it: {missed_unshifted}")
    assert inside_total > 100000 and missed == 0
    assert missed_unshifted > 0


def test_seg_tables_order_colours_and_truncation(sp):
    palette = sp.DEFAULT_PALETTE
    annot = [obj([10.9, 5.2, 30.5, 6.7, 20.1, 25.99], [-3.7, -0.5, 12.2, 3.9, 4.4, 18.6, 1.5, 9.5]), obj([1, 1, 9, 2]), obj([4, 4]),
             obj([40, 10, 60, 10, 60, 30, 40, 30])]
    shapes, toggles = sp.seg_tables(annot, 50, 70)
    kinds = shapes[:, 0].tolist()
    assert kinds == [sr.FILL] + [sr.LINE] * 3 + [sr.FILL] + [sr.LINE] * 4 + [sr.LINE] * 2 + [sr.LINE] + [sr.FILL] + [sr.LINE] * 4
    colour = lambda i: int(palette[i][0]) | int(palette[i][1]) << 8 | int(palette[i][2]) << 16  # noqa: E731
    assert shapes[:, 1].tolist() == [colour(0)] * 9 + [colour(1)] * 2 + [colour(2)] + [colour(3)] * 5
    assert (shapes[:, 6:] == 0).all() and shapes.dtype == np.int32 and toggles.dtype == np.uint32
    # truncation toward zero, also below zero: -3.7 -> -3, -0.5 -> 0; closed contours: vertex j -> j + 1, last -> first
    assert shapes[1:4, 2:6].tolist() == [[10, 5, 30, 6], [30, 6, 20, 25], [20, 25, 10, 5]]
    assert shapes[5:9, 2:6].tolist() == [[-3, 0, 12, 3], [12, 3, 4, 18], [4, 18, 1, 9], [1, 9, -3, 0]]
    assert shapes[9:11, 2:6].tolist() == [[1, 1, 9, 2], [9, 2, 1, 1]] and shapes[11, 2:6].tolist() == [4, 4, 4, 4]
    # the fills index one toggle table, back to back, and are the polygon rule of the truncated vertices plus 0.5
    fills = shapes[shapes[:, 0] == sr.FILL]
    assert fills[0, 2] == 0 and fills[1, 2] == fills[0, 3] and fills[2, 2] == fills[1, 2] + fills[1, 3] and fills[2, 2] + fills[2, 3] == len(toggles)
    from_lib = sp.cm.polygon_toggles([10.5, 5.5, 30.5, 6.5, 20.5, 25.5], 50, 70)
    assert np.array_equal(toggles[:fills[0, 3]], from_lib)
    square = sr.fill_mask(toggles[fills[2, 2]:], 50, 70)
    # the square 40..60 x 10..30: the shifted fill holds the pixels 41..60 x 11..30, the contour draws the columns 40, 60 and rows 10, 30
    assert square[11:31, 41:61].all() and square.sum() == 400
    assert sr.covered(shapes[-5:], toggles, 50, 70).sum() == 21 * 21
    polys = sp.recorded_polygons(shapes)
    assert [len(v) for _, v in polys] == [3, 4, 2, 1, 4] and polys[1][0] == tuple(int(c) for c in palette[0])
    with pytest.raises(ValueError):
        sp.seg_tables([obj([1, 2, 3, 4, 5])], 50, 70)                      # an odd count
    with pytest.raises(IndexError):
        sp.seg_tables([obj([1, 2, 3, 4, 9, 9])] * 3, 50, 70, palette=palette[:2])   # get_color's IndexError
    with pytest.raises(IndexError):
        sp.seg_tables([obj([1, 2, 3, 4, 9, 9])] * 101, 50, 70)
    mask = np.zeros((50, 70), bool)
    mask[5:20, 8:30] = True
    shapes, toggles = sp.seg_tables([rle_obj(mask)], 50, 70)
    assert shapes[:, 0].tolist() == [sr.FILL] and np.array_equal(sr.fill_mask(toggles, 50, 70), mask)
    assert shapes[0, 4:6].tolist() == [8, 29]
    with pytest.raises(ValueError):
        sp.seg_tables([rle_obj(mask)], 50, 71)
    assert sp.seg_tables([], 5, 5)[0].shape == (0, 8)


def _err(lib):
    return lib.hh_last_error().decode()


def test_refusals_before_any_device_call(pkg, sp):
    """Every refusal returns on the host from the HOST copies: the non-null 'device' addresses are never dereferenced or passed on."""
    lib = pkg._lib.load()
    fake = 0x1000
    fn = "hh_seg_overlay_u8_batch"

    def call(n=1, base=fake, ddev=fake, sdev=fake, tdev=fake, host=True, shost=True, thost=True, num=None, ntog=None, shape=None, toggles=None, row=1, **over):
        d = np.zeros(max(n, 1), sp.DESC)
        d["h"], d["w"], d["dst_offset"], d["w0"], d["w1"] = 8, 8, 4096, 0.6, 0.4
        t = np.array([9, 20] if toggles is None else toggles, np.uint32)  # 8 x 8: column 1 row 1 .. column 2 row 3
        s = np.array([[sr.FILL, 0x010203, 0, len(t), 1, 2, 0, 0], [sr.LINE, 0x040506, -3, 2, 11, 5, 0, 0]], np.int32)
        for k, v in (shape or {}).items():
            s[row, k] = v
        d["prim_count"] = len(s)
        for k, v in over.items():
            d[k][-1] = v
        return lib.hh_seg_overlay_u8_batch(base, ddev, d.ctypes.data if host else None, sdev, s.ctypes.data if shost else None, len(s) if num is None else num,
                                           tdev, t.ctypes.data if thost and len(t) else None, len(t) if ntog is None else ntog, n, None)

    for kw in (dict(base=None), dict(ddev=None), dict(host=False), dict(sdev=None), dict(shost=False), dict(tdev=None), dict(thost=False), dict(n=0), dict(n=-1),
               dict(n=65536), dict(num=-1), dict(ntog=-1), dict(ddev=fake + 4), dict(sdev=fake + 2), dict(tdev=fake + 1)):
        assert call(**kw) != 0 and fn in _err(lib), kw
    for kw, word in ((dict(h=0), "size"), (dict(w=16385), "size"), (dict(h=-3), "size"), (dict(src_offset=-1), "negative offset"),
                     (dict(dst_offset=-8), "negative offset"), (dict(dst_offset=100), "overlaps"), (dict(src_offset=4096 + 191), "overlaps"),
                     (dict(prim_offset=1), "outside the table"), (dict(prim_offset=-1), "outside the table"), (dict(prim_count=3), "outside the table"),
                     (dict(prim_count=-1), "outside the table"), (dict(num=1), "outside the table"),
                     (dict(w0=float("nan")), "finite"), (dict(w1=float("inf")), "finite"), (dict(flags=2), "flag"), (dict(reserved=1), "reserved"),
                     (dict(shape={0: 2}), "kind"), (dict(shape={0: -1}), "kind"), (dict(shape={1: 0x1000000}), "colour"), (dict(shape={1: -1}), "colour"),
                     (dict(shape={6: 1}), "reserved"), (dict(shape={7: -1}), "reserved"),
                     (dict(shape={2: (1 << 23) + 1}), "2^23"), (dict(shape={5: -(1 << 23) - 1}), "2^23"),
                     (dict(row=0, shape={2: 1}), "toggle range"), (dict(row=0, shape={3: 3}), "toggle range"), (dict(row=0, shape={2: -1}), "toggle range"),
                     (dict(ntog=1), "toggle range"), (dict(toggles=[20, 9]), "increasing"), (dict(toggles=[9, 9]), "increasing"),
                     (dict(toggles=[9, 65]), "h*w"), (dict(row=0, shape={4: 2}), "does not hold"), (dict(row=0, shape={5: 1}), "does not hold"),
                     (dict(row=0, shape={4: -1}), "column range"), (dict(row=0, shape={5: 8}), "column range"), (dict(row=0, shape={4: 3, 5: 2}), "column range")):
        assert call(**kw) != 0 and word in _err(lib), (kw, _err(lib))
    assert call(n=3, h=0) != 0 and "frame 2" in _err(lib)  # the last of three frames
    # in place (dst == src) is not an overlap, and an odd toggle count covers through the last column: both pass the checks (and would
    # launch: so they are checked on the host twin, which validates the same way)
    image = np.zeros((8, 8, 3), np.uint8)
    sp.overlay_host(image, [[sr.FILL, 1, 0, 1, 1, 7, 0, 0]], [9], in_place=True)
    with pytest.raises(pkg._lib.HHError, match="does not hold"):
        sp.overlay_host(image, [[sr.FILL, 1, 0, 1, 1, 6, 0, 0]], [9])
    rows = np.zeros((sp.MAX_SHAPES + 1, 8), np.int32)
    rows[:, 0] = sr.LINE
    with pytest.raises(pkg._lib.HHError, match="HH_SEG_MAX_SHAPES"):   # refused, never capped
        sp.overlay_host(image, rows, [])
    assert np.array_equal(sp.overlay_host(image, rows[:-1], []), sp.overlay_host(image, rows[:1], []))  # exactly the limit is drawn


def test_letterbox_and_plans_are_plain_data(sp):
    assert sp.letterbox(100, 200, 160) == (80, 160, 40, 0) and sp.letterbox(200, 100, 160) == (160, 80, 0, 40)
    assert sp.letterbox(3, 2, 5) == (5, 3, 0, 1)          # 2 * 5 / 3 = 3.33 -> 3
    assert sp.letterbox(2, 4, 5) == (2, 5, 1, 0)          # 2 * 1.25 = 2.5 -> 2: half to even
    assert sp.letterbox(6, 4, 5) == (5, 3, 0, 1)          # 4 * 5 / 6 = 3.33
    assert sp.letterbox(163, 163, 163) == (163, 163, 0, 0)
    plan = sp.plan_raw(100, 200, [obj([10, 10, 50, 12, 30, 60])], 163)
    assert plan["size"] == (163, 163) and plan["labels"] == ["Raw Image", "Shape: 100 x 200"]
    assert plan["weights"] == (np.float32(0.6), np.float32(0.4)) and len(plan["prims"]) == 0


def test_plotting_needs_the_gpu(pkg, sp, monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(pkg._lib.HHError):
        sp.plot_segmentations(np.zeros((8, 8, 3), np.uint8), [])
    with pytest.raises(pkg._lib.HHError):
        sp.plot_raw(np.zeros((8, 8, 3), np.uint8), [], 16)


# ---------------------------------------------------------------------------------------------------------------- the golden
def _plan_of(sp, case):
    from sample_plot_helpers import STAGE_SIZES, golden_items
    raw, annot, sample, stem = golden_items()[case["idx"]]
    kw = dict(case["kwargs"])
    plan = sp.plan_sample(raw.shape[:2], annot, [(s, s) for s in STAGE_SIZES], sample[3], stem, nrows=kw.get("nrows", 3), stage_idxs=tuple(kw.get("stage_idxs", (1,))))
    return plan, raw, annot, sample


def test_cases_of_the_golden(sample_golden):
    from sample_plot_helpers import golden_items
    meta, _ = sample_golden
    items = golden_items()
    assert {tuple(i[0].shape[:2]) for i in items} == {(90, 140), (120, 80)}                       # two aspects
    assert any(len(o["segmentation"]) == 2 for o in items[0][1]) and any(o["num_keypoints"] == 0 for o in items[0][1])
    assert all(isinstance(o["segmentation"], list) for i in items for o in i[1])                     # polygon objects only
    assert [c["tag"] for c in meta["samples"]] == ["plot_default", "examples_0", "examples_1"]
    assert meta["samples"][0]["kwargs"] == {} and meta["samples"][1]["kwargs"] == {"nrows": 1, "stage_idxs": [1, 0]}


@pytest.mark.parametrize("n", [0, 1, 2])
def test_plan_sample_equals_the_golden(pkg, sp, sample_golden, n):
    """What the reference's own plot / plot_raw did, call by call, against plan_sample / plan_raw."""
    import render_ref as rr
    meta, data = sample_golden
    case = meta["samples"][n]
    vis, tx = pkg.keypoints.visualization, pkg.keypoints.text
    plan, raw, annot, sample = _plan_of(sp, case)
    stages, rp = plan["stages"], plan["raw"]
    K = len(meta["labels"])
    assert sp.COCO_LABELS == meta["labels"] and [list(l) for l in sp.COCO_LIMBS] == meta["limbs"]
    assert list(plan["size"]) == case["size"]
    # every cv2.resize: the model input to each stage's size, then make_grid's match_size on every stage grid
    mh, mw = plan["matched"]
    assert case["resizes"] == [[128, 128, st["size"][1], st["size"][0]] for st in stages] + [[*st["grid"], mw, mh] for st in stages]
    # plot_heatmaps: the resized image before the skeleton, the stage's target maps as they are, no clip, no minmax
    for st, rec in zip(stages, case["heatmaps"]):
        hms = sample[1][st["stage"]]
        assert rec == dict(image_is_the_resized_input=True, shape=[K, *st["size"]], sum=float(np.float64(hms).sum()), kwargs={})
    # plot_connections: one call per stage, then the raw pane's
    assert case["skeletons"] == len(stages) + 1
    joint_sets = [np.asarray(sample[3][st["stage"]], np.float64) for st in stages] + [sp.annot_joints(annot)]
    for k, (joints, prims) in enumerate(zip(joint_sets, [st["prims"] for st in stages] + [rp["prims"]])):
        table, dirs = vis.build_primitives(joints[..., :2], joints[..., 2], sp.COCO_LIMBS, 0.5, "person", return_direction=True)
        assert np.array_equal(table, prims) and len(table) > 0
        assert rr.same_calls(rr.calls_of_table(table, dirs, 0.8), data[f"{case['tag']}.skeleton{k}"]), k
    # every put_txt call: the cell, the box, the weights, the strings and their origins
    calls = [(st, c) for st in stages for c in st["text_calls"]]
    assert len(case["puts"]) == len(calls) + 1
    frames = [(st["size"], c) for st, c in calls] + [(rp["size"], (-1, rp["labels"], 1.0, 0.5))]
    for rec, ((h, w), (cell, labels, alpha, fs)) in zip(case["puts"], frames):
        _, lay = tx.layout_put_txt(h, w, labels, alpha=alpha, font_scale=fs, return_layout=True)
        box = list(lay["box"]) if lay["opaque"] else [max(lay["box"][0], 0), max(lay["box"][1], 0), min(lay["box"][2], w - 1), min(lay["box"][3], h - 1)]
        assert (rec["cell"], rec["frame"], rec["strings"], rec["font_scale"]) == (cell, [h, w], list(labels), fs)
        assert (rec["box"], rec["opaque"], rec["weights"]) == (box, int(lay["opaque"]), [1.0 - alpha, float(alpha)] if not lay["opaque"] else [0.0, 1.0])
        assert rec["origins"] == [list(o) for o in lay["origins"]] and rec["bg_color"] == list(lay["bg_color"]) and rec["txt_color"] == list(lay["txt_color"])
    for st in stages:
        tables = [sp._shift(tx.layout_put_txt(*st["size"], lab, alpha=a, font_scale=fs), *st["cells"][cell]) for cell, lab, a, fs in st["text_calls"]]
        assert np.array_equal(st["text"], np.concatenate(tables))
    assert np.array_equal(rp["text"], tx.layout_put_txt(*rp["size"], rp["labels"]))
    # the polygons as cv2 received them: fillPoly then drawContours(thickness 1) per polygon, truncated vertices, the object's colour
    fills, contours = case["polygons"][0::2], case["polygons"][1::2]
    assert all(f["call"] == "fillPoly" and c["call"] == "drawContours" and c["thickness"] == 1 and f["vertices"] == c["vertices"] and f["colour"] == c["colour"]
               for f, c in zip(fills, contours)) and len(fills) == len(contours) == sum(len(o["segmentation"]) for o in annot)
    mine = sp.recorded_polygons(rp["shapes"])
    assert [(list(c), v.tolist()) for c, v in mine] == [(c["colour"], c["vertices"]) for c in contours]
    kinds = rp["shapes"][:, 0].tolist()
    assert kinds == [k for c in contours for k in [sr.FILL] + [sr.LINE] * len(c["vertices"])]
    w_overlay, w_image = case["overlay_weights"]
    assert rp["weights"] == (np.float32(w_image), np.float32(w_overlay)) and rp["overlay_alpha"] == w_overlay
    # the letterbox parameters (the arithmetic behind `restated` is this project's on both sides: UNPINNED against albumentations)
    lb = case["letterbox"]
    assert lb["max_size"] == lb["min_height"] == lb["min_width"] == plan["model_grid"][0] == rp["size"][0] == rp["size"][1]
    assert lb["image"] == list(raw.shape[:2]) == list(rp["raw_size"]) and lb["restated"] == list(rp["letterbox"])
    # the grids
    for st, g in zip(stages, case["grids"]):
        assert g["fn"] == "make_grid" and g["kwargs"] == {"nrows": case["kwargs"].get("nrows", 3)} and g["inputs"] == [list(st["size"])] * (2 + K)
        assert g["places"] == [[y, x, *st["size"]] for y, x in st["cells"]] and g["out"] == list(st["grid"])
    g = case["grids"][len(stages)]
    assert g["kwargs"] == {"nrows": len(stages), "match_size": 1} and g["inputs"] == [list(st["grid"]) for st in stages]
    assert g["places"] == [[y, x, mh, mw] for y, x in plan["model_places"]] and g["out"] == list(plan["model_grid"])
    g = case["grids"][len(stages) + 1]
    Gh, Gw = plan["model_grid"]
    assert g["fn"] == "stack_horizontally" and g["places"] == [[*plan["stack"][0], Gh, Gh], [*plan["stack"][1], Gh, Gw]] and g["out"] == list(plan["size"])
    assert len(case["grids"]) == len(stages) + 2


def test_plan_examples_equals_the_golden(sp, sample_golden):
    meta, _ = sample_golden
    ex = meta["examples"]
    plan = sp.plan_examples(ex["grid"]["inputs"])
    assert ex["grid"]["kwargs"] == {"nrows": 2, "pad": 20}
    assert [[y, x, *ex["grid"]["inputs"][0]] for y, x in plan["places"]] == ex["grid"]["places"] and list(plan["size"]) == ex["size"] == ex["grid"]["out"]
    with pytest.raises(ValueError):
        sp.plan_examples([(10, 20), (10, 21)])


def test_golden_regenerates_bit_for_bit(tmp_path):
    """tools/make_sample_plot_golden.py, run over the checkout of the reference where the golden tools look for it (HH_REFERENCE names
    another place), reproduces the committed files.  A missing checkout fails: the non-GPU suite runs where the fixtures are made."""
    ref = os.environ.get("HH_REFERENCE", "/root/reference")
    assert os.path.isdir(os.path.join(ref, "src", "keypoints")), f"{ref} is no checkout of the reference (HH_REFERENCE names another place)"
    subprocess.check_call([sys.executable, os.path.join(REPO, "tools", "make_sample_plot_golden.py"), ref, str(tmp_path)], stdout=subprocess.DEVNULL,
                          env=dict(os.environ, PYTHONDONTWRITEBYTECODE="1"))
    assert open(tmp_path / "sample_plot_meta.json").read() == open(os.path.join(GOLDEN, "sample_plot_meta.json")).read()
    new, old = np.load(tmp_path / "sample_plot.npz"), np.load(os.path.join(GOLDEN, "sample_plot.npz"))
    # (the arrays bit for bit; the archive around them carries the time it was written)
    assert sorted(new.files) == sorted(old.files) and all(new[k].dtype == old[k].dtype and new[k].tobytes() == old[k].tobytes() for k in old.files)
