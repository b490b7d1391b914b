"""Host half of the pose overlay (keypoints/visualization.py, hh_render_poses_u8_batch, hh_resize_u8): no GPU needed.

The golden (tests/golden/render.npz, tools/make_render_golden.py) was produced by the reference's own plot_connections / draw_elipsis /
get_color; cv2.ellipse, cv2.circle and cv2.addWeighted were bound to the recorders of tests/render_ref.py (log + the project's stated
rasterisation rule: parity of the covered pixels with cv2 itself is UNPINNED, see the fixture's meta and include/hhrnet.h).

The recorded angle is compared within 1e-9 degrees to atan2(s, c) of the float64 direction that build_primitives forms (its
`return_direction` output); the table itself holds that direction rounded once to fp32, as the rule states, which the test checks
exactly.  (atan2 of the fp32 pair would be off by up to 2^-24 rad = 3.4e-6 degrees.)"""
import numpy as np
import pytest

import render_ref as rr
from render_helpers import MAX_PRIMS, case_inputs, lattice, reference, render_golden, vis  # noqa: F401

def test_abi_and_exports(pkg):
    lib = pkg._lib.load()
    assert lib.hh_abi_version() == 3
    for name in ("hh_render_poses_u8_batch", "hh_render_config", "hh_debug_render_host", "hh_resize_u8"):
        assert hasattr(lib, name) and name in pkg._lib.exported_symbols(), name
    Th, Tw, chunk, px = pkg.keypoints.visualization.render_config()
    assert Th >= 1 and Tw >= 1 and chunk >= 1 and px >= 1 and Tw % px == 0


def test_cases_cover_the_issue(render_golden):
    meta, data = render_golden
    cases = meta["cases"]
    assert {c["color_mode"] for c in cases} == {"person", "limb"}
    assert {c["alpha"] for c in cases} >= {0.0, 0.65, 0.8, 1.0}
    assert {c["people"] for c in cases} >= {0, 1, 3, 30}
    coords, scores = data["edges_person.coords"], data["edges_person.scores"]
    thr = meta["thr"]
    assert (scores == thr).any() and (scores[1] < thr).all()
    xy = np.trunc(coords[2]).astype(int)
    limbs = meta["limbs"]
    d = np.array([xy[b] - xy[a] for a, b in limbs])
    assert (d == 0).all(1).any()                                            # both ends on one pixel
    assert ((abs(d[:, 0]) == abs(d[:, 1])) & (d[:, 0] != 0)).any()          # |dx| == |dy|
    assert {(int(np.sign(x)), int(np.sign(y))) for x, y in d} >= {(1, 1), (1, -1), (-1, 1), (-1, -1)}        # all four quadrants
    assert ((d[:, 0] == 0) & (d[:, 1] != 0)).any() and ((d[:, 1] == 0) & (d[:, 0] != 0)).any()   # axis-aligned both ways
    sums = np.array([xy[a] + xy[b] for a, b in limbs])
    assert ((sums < 0) & (sums % 2 == 1)).any()                             # a floor of a negative odd sum
    assert (coords[2] < 0).any() and (coords[2, :, 0] > meta["frame"][1]).any()
    assert int((coords[3, :, 1].max() - coords[3, :, 1].min()) / 100) > 2   # s_i > 2
    frac = coords[2] - np.floor(coords[2])
    assert (frac > 0.999999).any()                                          # just below an integer


def test_render_ref_reproduces_golden(render_golden):
    meta, data = render_golden
    for c in meta["cases"]:
        img, coords, scores = case_inputs(data, c)
        got = rr.render(img, coords, scores, meta["limbs"], c["thr"], c["color_mode"], c["alpha"], data["get_color"])
        assert np.array_equal(got, data[c["tag"] + ".out"]), c["tag"]
        assert int((got != img).any(-1).sum()) == c["changed_pixels"]


def test_default_palette_is_get_color(vis, render_golden):
    _, data = render_golden
    assert vis.DEFAULT_PALETTE.dtype == np.uint8 and np.array_equal(vis.DEFAULT_PALETTE, data["get_color"])
    assert np.array_equal(vis.DEFAULT_PALETTE[:20], vis.DEFAULT_PALETTE[80:])


def test_build_primitives_equals_recorded_calls(vis, render_golden):
    meta, data = render_golden
    worst = 0.0
    for c in meta["cases"]:
        img, coords, scores = case_inputs(data, c)
        table, dirs = vis.build_primitives(coords, scores, meta["limbs"], c["thr"], c["color_mode"], vis.DEFAULT_PALETTE, c["alpha"], return_direction=True)
        rec = data[c["tag"] + ".calls"]
        mine = rr.calls_of_table(table, dirs, c["alpha"])
        assert mine.shape == rec.shape == (c["calls"], 10), c["tag"]
        other = [k for k in range(10) if k != rr.ANGLE_COL]
        assert np.array_equal(mine[:, other], rec[:, other]), c["tag"]          # every field but the angle: exact
        # the angle is taken modulo 360: the reference's arctan2 and atan2(s, c) are the same function of the same quadrant
        diff = np.abs((mine[:, rr.ANGLE_COL] - rec[:, rr.ANGLE_COL] + 180.0) % 360.0 - 180.0)
        worst = max(worst, float(diff.max()))
        assert diff.max() <= 1e-9, (c["tag"], diff.max())
        assert np.array_equal(table["c"], dirs[:, 0].astype(np.float32)) and np.array_equal(table["s"], dirs[:, 1].astype(np.float32))
        w0, w1 = vis.blend_weights(c["alpha"])
        assert w0 == np.float32(rec[-1, 1]) and w1 == np.float32(rec[-1, 2])
    print(f"worst angle difference {worst:.3e} degrees")


def test_build_primitives_edges(vis):
    assert len(vis.build_primitives(np.zeros((0, 17, 2)), np.zeros((0, 17)), rr.COCO_LIMBS, 0.05, "person")) == 0
    coords, scores = np.zeros((3, 17, 2)) + 5.0, np.ones((3, 17))
    with pytest.raises(IndexError):
        vis.build_primitives(coords, scores, rr.COCO_LIMBS, 0.05, "person", vis.DEFAULT_PALETTE[:2])
    with pytest.raises(IndexError):
        vis.build_primitives(coords, scores, rr.COCO_LIMBS, 0.05, "limb", vis.DEFAULT_PALETTE[:18])
    assert len(vis.build_primitives(coords, scores, rr.COCO_LIMBS, 0.05, "limb", vis.DEFAULT_PALETTE[:19])) == 3 * (19 + 34)
    with pytest.raises(IndexError):
        vis.build_primitives(np.zeros((101, 17, 2)), np.ones((101, 17)), None, 0.05, "person")
    with pytest.raises(ValueError):
        vis.build_primitives(coords * 1e7, scores, rr.COCO_LIMBS, 0.05, "person")
    with pytest.raises(ValueError):
        vis.build_primitives(coords, scores, rr.COCO_LIMBS, 0.05, "rainbow")
    t = vis.build_primitives(coords, scores[..., None], None, 0.05, "person")   # [P,K,1] scores, no limbs
    assert len(t) == 3 * 34 and t.dtype.itemsize == 32


DEFECTS = {  # defect -> a golden case on which it must show
    "ring_first": "person_a08", "reverse_people": "crowd30", "trunc_centre": "edges_person", "swap_axes": "person_a08", "strict_thr": "edges_person",
    "size_from_drawn": "edges_limb", "kpts_first": "limb_a065",
}
# Defects that no frame can show under the stated rasterisation, on any input: the stated disc (dx^2 + dy^2 <= r^2 + r) and the stated ring
# of the same keypoint (R = r + 1: R^2 - R < dx^2 + dy^2 <= R^2 + R, and R^2 - R = r^2 + r identically) cover disjoint pixel sets, so which
# of the two is drawn first cannot change a pixel (test_disc_and_ring_of_one_keypoint_are_disjoint; it would under cv2's midpoint
# circles).  The golden still tells this defect from the rule, through the call list the reference's own function left in it.
NO_PIXEL_CAN_SHOW = ("ring_first",)


@pytest.mark.parametrize("defect", sorted(DEFECTS))
def test_planted_defect_shows(render_golden, defect):
    """Each planted variant of the rule must differ from the golden (recorded call list + output image) on its named case, or the
    cases do not discriminate.  Every variant must differ from the recorded call list, which the unplanted rule reproduces; every
    variant must differ in the output image as well, except where the rule itself makes that impossible (NO_PIXEL_CAN_SHOW), and
    there the image must be equal, so that the exception cannot hide a second defect."""
    meta, data = render_golden
    c = next(c for c in meta["cases"] if c["tag"] == DEFECTS[defect])
    img, coords, scores = case_inputs(data, c)
    args = (coords, scores, meta["limbs"], c["thr"], c["color_mode"], data["get_color"])
    recorded = data[c["tag"] + ".calls"]
    assert rr.same_calls(rr.calls_of_prims(rr.primitives(*args), c["alpha"]), recorded), "the rule itself does not reproduce the recorded calls"
    assert not rr.same_calls(rr.calls_of_prims(rr.primitives(*args, **{defect: True}), c["alpha"]), recorded), f"{defect}: same calls on {c['tag']}"
    got = rr.render(img, coords, scores, meta["limbs"], c["thr"], c["color_mode"], c["alpha"], data["get_color"], **{defect: True})
    if defect in NO_PIXEL_CAN_SHOW:
        assert np.array_equal(got, data[c["tag"] + ".out"]), f"{defect} changes pixels on {c['tag']}: the rule's sets are not disjoint"
    else:
        assert not np.array_equal(got, data[c["tag"] + ".out"]), f"{defect} does not show on {c['tag']}"


def test_disc_and_ring_of_one_keypoint_are_disjoint():
    for r in (1, 2, 3, 7, 40):
        disc, ring = rr.disc_mask(101, 103, 50, 51, r), rr.ring_mask(101, 103, 50, 51, r + 1)
        assert disc.any() and ring.any() and not (disc & ring).any()
        assert np.array_equal(disc | ring, rr.disc_mask(101, 103, 50, 51, r + 1))   # together: the disc of radius r + 1


def test_host_walk_equals_render_ref(vis, render_golden):
    """hh_debug_render_host (the kernel's tile walk, boxes and chunks, compiled for the host) against the rule on whole frames."""
    meta, data = render_golden
    for c in meta["cases"]:
        img, coords, scores = case_inputs(data, c)
        table = vis.build_primitives(coords, scores, meta["limbs"], c["thr"], c["color_mode"], vis.DEFAULT_PALETTE, c["alpha"])
        assert np.array_equal(vis.render_host(img, table, c["alpha"]), data[c["tag"] + ".out"]), c["tag"]
        assert np.array_equal(vis.render_host(img, table, c["alpha"], bgr=True), data[c["tag"] + ".out"][..., ::-1]), c["tag"]
    for name, img, table, alpha, bgr in lattice(vis, vis.render_config()):
        assert np.array_equal(vis.render_host(img, table, alpha, bgr), reference(img, table, alpha, bgr)), name


def _ellipses(vis, render_golden):
    meta, data = render_golden
    for c in meta["cases"]:
        img, coords, scores = case_inputs(data, c)
        table = vis.build_primitives(coords, scores, meta["limbs"], c["thr"], c["color_mode"], vis.DEFAULT_PALETTE, c["alpha"])
        yield from ((img.shape[:2], p) for p in rr.from_table(table) if p[0] == rr.ELLIPSE)
    for name, img, table, alpha, bgr in lattice(vis, vis.render_config()):
        if name.startswith("stack_") and not name.endswith(f"_{vis.render_config()[2]}"):
            continue  # (the stacks repeat the same ellipses: one of them is enough)
        yield from ((img.shape[:2], p) for p in rr.from_table(table) if p[0] == rr.ELLIPSE)


def test_fp32_ellipse_against_float64(vis, render_golden):
    """The fp32 inside test may differ from the same inequality in float64 (same fp32-rounded c, s) only where the float64 margin
    |lhs - rhs| / rhs is within what the stated operation order can lose.  With e = 2^-24 (round to nearest) and exact (float)dx,
    (float)dy, A, B:
      t0 = dx c, t1 = dy s, u = t0 + t1:   |du| <= e (|t0| + |t1|) + e |u|       (two products, one sum; likewise dv from t2, t3)
      p = (2u) B (2u exact):               |dp| <= 2 B |du| + e |p|              (likewise dq with A)
      p^2, q^2:                            |d(p^2)| <= 2 |p| |dp| + e p^2
      lhs = p^2 + q^2:                     |dlhs| <= |d(p^2)| + |d(q^2)| + e (p^2 + q^2)
      rhs = (A B)^2:                       |drhs| <= 3 e rhs                      (one product, then its square)
    to first order in e; the second-order terms are below e times these and are covered by the factor 1.001.  A decision can flip only
    if |lhs - rhs| <= |dlhs| + |drhs|.  Prints the worst margin / bound over the disagreeing pixels and fails above 1."""
    e = 2.0 ** -24
    worst, flips, tested = 0.0, 0, 0
    for (h, w), (_, cx, cy, a, b, c, s, _) in _ellipses(vis, render_golden):
        l32, r32 = rr.ellipse_terms(h, w, cx, cy, a, b, c, s, np.float32)
        l64, r64 = rr.ellipse_terms(h, w, cx, cy, a, b, c, s, np.float64)
        dy, dx = np.mgrid[0:h, 0:w].astype(np.float64)
        dx, dy, c, s, A, B = dx - cx, dy - cy, float(c), float(s), 2.0 * a + 1, 2.0 * b + 1
        u, v = dx * c + dy * s, dy * c - dx * s
        du = e * (abs(dx * c) + abs(dy * s)) + e * abs(u)
        dv = e * (abs(dy * c) + abs(dx * s)) + e * abs(v)
        p, q = 2 * u * B, 2 * v * A
        dp, dq = 2 * B * du + e * abs(p), 2 * A * dv + e * abs(q)
        dl = 2 * abs(p) * dp + e * p * p + 2 * abs(q) * dq + e * q * q + e * (p * p + q * q)
        bound = 1.001 * (dl + 3 * e * r64) / r64
        differ = (l32 <= r32) != (l64 <= r64)
        tested += differ.size
        if differ.any():
            flips += int(differ.sum())
            margin = abs(l64 - r64) / r64
            worst = max(worst, float((margin[differ] / bound[differ]).max()))
    print(f"fp32 / float64 ellipse test: {flips} disagreeing pixels of {tested} tested, worst margin / bound {worst:.3f}")
    assert worst <= 1.0


def _err(lib):
    return lib.hh_last_error().decode()


def test_render_refusals_before_any_device_call(pkg, vis):
    """Every refusal returns on the host from the HOST copies: the non-null 'device' addresses are never dereferenced or passed on."""
    lib = pkg._lib.load()
    fake = 0x1000

    def call(n=1, prims=None, num=None, base=fake, ddev=fake, pdev=fake, host=True, phost=True, **over):
        d = np.zeros(max(n, 1), vis.DESC)
        d["h"], d["w"], d["dst_offset"], d["w0"], d["w1"] = 8, 8, 4096, 0.2, 0.8
        table = vis.table_of([vis.circle_prim(3, 3, 2, (1, 2, 3))] if prims is None else prims)
        d["prim_count"] = len(table)
        for k, v in over.pop("prim", {}).items():
            table[k] = v
        for k, v in over.items():
            d[k][-1] = v
        return lib.hh_render_poses_u8_batch(base, ddev, d.ctypes.data if host else None, pdev, table.ctypes.data if phost and len(table) else None,
                                            len(table) if num is None else num, n, None)

    for kw in (dict(base=None), dict(ddev=None), dict(host=False), dict(pdev=None), dict(phost=False), dict(n=0), dict(n=-1), dict(n=65536), dict(num=-1),
               dict(ddev=fake + 4), dict(pdev=fake + 2)):
        assert call(**kw) != 0 and "hh_render_poses_u8_batch" in _err(lib), kw
    for kw, word in ((dict(h=0), "size"), (dict(w=16385), "size"), (dict(h=-3), "size"), (dict(src_offset=-1), "negative offset"),
                     (dict(dst_offset=-8), "negative offset"), (dict(prim_offset=1), "outside the table"), (dict(prim_offset=-1), "outside the table"),
                     (dict(prim_count=2), "outside the table"), (dict(prim_count=-1), "outside the table"), (dict(num=0), "outside the table"),
                     (dict(w0=float("nan")), "finite"), (dict(w1=float("inf")), "finite"), (dict(flags=2), "flag"),
                     (dict(prim=dict(kind=3)), "kind"), (dict(prim=dict(A=0)), "A or B"), (dict(prim=dict(B=0)), "A or B"),
                     (dict(prim=dict(A=40000)), "radius"), (dict(prim=dict(cx=1 << 24)), "centre"), (dict(prim=dict(cy=-(1 << 24))), "centre"),
                     (dict(prim=dict(x0=-1, y0=0, x1=5, y1=5)), "box"), (dict(prim=dict(x0=0, y0=0, x1=16384, y1=5)), "box"),
                     (dict(prim=dict(cx=-40000, x0=0, y0=0, x1=5, y1=5)), "too far")):
        assert call(**kw) != 0 and word in _err(lib), (kw, _err(lib))
    assert call(n=3, h=0) != 0 and "frame 2" in _err(lib)  # the last of three frames
    rows = [vis.circle_prim(3, 3, 2, (1, 2, 3))] * (MAX_PRIMS + 1)
    assert call(prims=rows) != 0 and "HH_RENDER_MAX_PRIMS" in _err(lib)  # refused, never capped
    # the same checks stand in front of the host walk
    img = np.zeros((8, 8, 3), np.uint8)
    with pytest.raises(pkg._lib.HHError, match="HH_RENDER_MAX_PRIMS"):
        vis.render_host(img, vis.table_of(rows), 0.8)


def test_resize_refusals_before_any_device_call(pkg):
    lib = pkg._lib.load()
    fake = 0x1000

    def call(src=fake, h=8, w=8, ch=3, dst=fake, H=4, W=4):
        return lib.hh_resize_u8(src, h, w, ch, dst, H, W, None)

    for kw, word in ((dict(src=None), "null"), (dict(dst=None), "null"), (dict(ch=2), "channels"), (dict(ch=4), "channels"), (dict(ch=0), "channels"),
                     (dict(h=0), "1..16384"), (dict(w=-1), "1..16384"), (dict(H=0), "1..16384"), (dict(W=16385), "1..16384"), (dict(h=16385), "1..16384")):
        assert call(**kw) != 0 and "hh_resize_u8" in _err(lib) and word in _err(lib), (kw, _err(lib))


def test_plot_connections_needs_the_gpu(pkg, monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(pkg._lib.HHError):
        pkg.keypoints.plot_connections(np.zeros((8, 8, 3), np.uint8), np.zeros((0, 17, 2)), np.zeros((0, 17)), rr.COCO_LIMBS, 0.05, "person", 0.8)
