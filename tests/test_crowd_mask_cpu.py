"""Host half of the crowd masks (keypoints/crowd_mask.py, hh_crowd_polygon_toggles, hh_debug_crowd_masks_host and the argument checks
of hh_crowd_masks_u8_batch): no GPU needed.

tests/crowd_mask_ref.py restates the rule of include/hhrnet.h in numpy and does not call the library.  The fixtures are the ones stated
with the rule (h = 8, w = 9); parity of the polygon conversion with the COCO API package itself is UNPINNED."""
import ctypes as C

import numpy as np
import pytest

import crowd_mask_ref as ref
from crowd_mask_helpers import (FIXTURES, H8, RECTANGLE, W9, cm, column_range, host_walk, lattice, person, picture,  # noqa: F401
                                stage_one)


def test_abi_and_exports(pkg, cm):
    lib = pkg._lib.load()
    assert lib.hh_abi_version() == 3
    for name in ("hh_crowd_polygon_toggles", "hh_crowd_polygon_capacity", "hh_crowd_masks_u8_batch", "hh_crowd_mask_config", "hh_debug_crowd_masks_host"):
        assert hasattr(lib, name) and name in pkg._lib.exported_symbols(), name
    th, tw, threads, chunk = cm.config()
    assert th >= 1 and tw >= 1 and threads >= 1 and chunk >= 0
    for name in ("CrowdSegments", "crowd_masks", "get_crowd_mask", "raw_sample"):
        assert hasattr(pkg.keypoints, name), name


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_restatement_reproduces_fixture(name):
    xy, emitted, pixels, rows = FIXTURES[name]
    if emitted is not None:
        assert len(ref.polygon_positions(xy, H8, W9)) == emitted
    t = ref.polygon_toggles(xy, H8, W9)
    assert t.dtype == np.uint32 and (np.diff(t.astype(np.int64)) > 0).all()
    cov = ref.covered(t, H8, W9)
    assert picture(cov) == list(rows) and int(cov.sum()) == pixels
    if name == "outside":
        assert t.size == 0


def test_restatement_small_cases():
    assert ref.covered(ref.polygon_toggles([0, 0, 0, 1, 1, 1, 1, 0], 1, 1), 1, 1).tolist() == [[True]]  # the unit square on 1 x 1
    # the clamp to h puts a toggle on the first position of the next column
    t = ref.polygon_toggles(FIXTURES["off_bottom"][0], H8, W9)
    assert (t % H8 == 0).any() and int(t[-1]) == 6 * H8


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_library_equals_restatement_on_fixtures(cm, name):
    xy = FIXTURES[name][0]
    assert np.array_equal(cm.polygon_toggles(xy, H8, W9), ref.polygon_toggles(xy, H8, W9))


def test_library_equals_restatement_on_lattice(pkg, cm):
    cases = lattice()
    assert len(cases) == 400
    partial = border = 0
    for h, w, xy in cases:
        want = ref.polygon_toggles(xy, h, w)
        got = cm.polygon_toggles(xy, h, w)
        assert got.dtype == np.uint32 and np.array_equal(got, want), (h, w, xy.tolist())
        cov = ref.covered(want, h, w)
        partial += 0 < cov.sum() < h * w
        border += bool(cov[0].any() or cov[-1].any() or cov[:, 0].any() or cov[:, -1].any())
        cap = pkg._lib.load().hh_crowd_polygon_capacity(xy.ctypes.data, len(xy) // 2, h, w)
        assert cap >= want.size
    print(f"lattice: {partial} of 400 neither empty nor full, {border} touch a border")
    assert partial >= 0.9 * len(cases) and border >= 0.5 * len(cases)  # the lattice cannot pass vacuously


def test_polygon_refusals(pkg, cm):
    lib = pkg._lib.load()
    out = np.zeros(64, np.uint32)

    def call(xy, k, h, w, cap=64):
        xy = np.asarray(xy, np.float64)
        before = out.copy()
        n = lib.hh_crowd_polygon_toggles(xy.ctypes.data, k, h, w, out.ctypes.data, cap)
        if n < 0:
            assert np.array_equal(out, before) and lib.hh_last_error().decode().startswith("hh_crowd_polygon_toggles: ")
            assert lib.hh_crowd_polygon_capacity(xy.ctypes.data, k, h, w) == -1 or cap < 64
        return n

    assert call(RECTANGLE, 4, 8, 9) == 8
    assert call(RECTANGLE, 2, 8, 9) == -1
    for bad in (np.nan, np.inf, -np.inf):
        assert call([0, 0, 0, 4, bad, 4, 4, 0], 4, 8, 9) == -1
    for h, w in ((0, 9), (8, 0), (16385, 9), (8, 16385), (-1, 9)):
        assert call(RECTANGLE, 4, h, w) == -1
    assert call([0, 0, 0, 4, 4.3e8, 4, 4, 0], 4, 8, 9) == -1     # 5 x leaves the int range
    assert call([0, 0, 0, 4, -4.3e8, 4, 4, 0], 4, 8, 9) == -1
    assert call(RECTANGLE, 4, 8, 9, cap=7) == -1 and "do not fit" in lib.hh_last_error().decode()
    assert lib.hh_crowd_polygon_toggles(None, 4, 8, 9, out.ctypes.data, 64) == -1
    with pytest.raises(ValueError):
        cm.polygon_toggles([0, 0, 1, 1], 8, 9)
    with pytest.raises(ValueError):
        cm.polygon_toggles([0, 0, 1, 1, 2, 2, 3], 8, 9)
    with pytest.raises(pkg._lib.HHError):
        cm.polygon_toggles([0, 0, 1, np.nan, 2, 2], 8, 9)


def test_host_walk_equals_mask_from_toggles(pkg, cm):
    th, tw, _, _ = cm.config()
    rng = np.random.RandomState(5)
    cases = [(H8, W9, [ref.polygon_toggles(FIXTURES[n][0], H8, W9) for n in ("triangle", "bow_tie", "off_right")]),
             (1, 1, [np.array([0], np.uint32)]), (1, 1, []), (3, 5, [np.array([15], np.uint32)]), (3, 5, [np.array([0, 15], np.uint32)])]
    for h, w in ((th - 1, tw - 1), (th, tw), (th + 1, tw + 1), (2 * th + 3, 7), (5, 2 * tw + 3)):
        lists = [np.unique(rng.randint(0, h * w + 1, rng.randint(1, 40))).astype(np.uint32) for _ in range(3)]
        cases.append((h, w, lists))
    for h, w, lists in cases:
        rc, got = host_walk(pkg, lists, h, w)
        assert rc == 0, pkg._lib.load().hh_last_error()
        assert np.array_equal(got, ref.mask_from_toggles(lists, h, w)), (h, w)


def test_run_length_cases(cm):
    h, w = 4, 5
    for counts in ([0, 3, 17], [2, 0, 0, 3, 15], [3, 0, 2, 0, 0, 1, 14], [1, 6, 2, 9, 2], [20], [0, 20], [5, 5, 0, 0, 10]):
        got = cm.rle_toggles(counts, h, w)
        assert got.dtype == np.uint32 and np.array_equal(got, ref.rle_toggles(counts, h, w)), counts
        # against the definition: runs alternate uncovered / covered over the column-major pixel order
        flat = np.concatenate([np.full(c, i % 2, bool) for i, c in enumerate(counts)])
        assert np.array_equal(ref.covered(got, h, w), flat.reshape(w, h).T), counts
    assert cm.rle_toggles([0, 3, 17], h, w).tolist() == [0, 3]            # a zero first run: covered from pixel 0
    assert cm.rle_toggles([2, 0, 0, 3, 15], h, w).tolist() == [2, 5]      # sums 2, 2, 2, 5: the triple stays once
    assert cm.rle_toggles([3, 0, 2, 0, 0, 1, 14], h, w).tolist() == [5, 6]  # 3, 3 cancel; 5, 5, 5 stays once
    assert cm.rle_toggles([1, 6, 2, 9, 2], h, w).tolist() == [1, 7, 9, 18]  # runs that span columns
    for bad in ([3, 16], [3, 18], [-1, 21], []):
        with pytest.raises(ValueError):
            cm.rle_toggles(bad, h, w)
    for bad in ("52203", b"52203"):
        with pytest.raises(ValueError):
            cm.rle_toggles(bad, h, w)
    with pytest.raises(ValueError):
        cm.segmentation_toggles({"counts": [3, 17], "size": [5, 4]}, h, w)  # size differs from the image


def test_validation_refusals_launch_nothing(pkg, cm):
    """Every refusal returns 1 with a message before anything is enqueued: the device pointers given here are not memory at all, and
    this machine may have no GPU."""
    lib = pkg._lib.load()
    h, w = 6, 7
    good = [np.array([3, 9, 20, 30], np.uint32), np.array([1], np.uint32)]
    fake_dev = 4096  # non-null, 4-byte aligned, never dereferenced

    def call(buf, md, sd, n=1, nseg=None, base=fake_dev, descs_dev=fake_dev, segs_dev=fake_dev, host_base="buf", descs_host="md", segs_host="sd"):
        nseg = len(sd) if nseg is None else nseg
        rc = lib.hh_crowd_masks_u8_batch(base, descs_dev, segs_dev, md.ctypes.data if descs_host == "md" else descs_host,
                                         sd.ctypes.data if segs_host == "sd" else segs_host, buf.ctypes.data if host_base == "buf" else host_base,
                                         n, nseg, None)
        assert rc == 1
        msg = lib.hh_last_error().decode()
        assert msg.startswith("hh_crowd_masks_u8_batch: "), msg
        return msg

    def staged(**edit):
        buf, md, sd = stage_one(cm, good, h, w)
        for key, value in edit.items():
            table, field, row = key.split("__")
            (md if table == "m" else sd)[field][int(row)] = value
        return buf, md, sd

    rc, _ = host_walk(pkg, good, h, w)
    assert rc == 0                                                       # the untouched tables are accepted
    assert "null pointer" in call(*staged(), base=None)
    assert "null pointer" in call(*staged(), descs_dev=None)
    assert "null pointer" in call(*staged(), segs_dev=None)
    assert "null pointer" in call(*staged(), descs_host=None)
    assert "null pointer" in call(*staged(), segs_host=None)
    assert "null pointer" in call(*staged(), host_base=None)
    assert "aligned" in call(*staged(), base=4098)
    for n in (0, -1, 65536):
        assert "n <= 65535" in call(*staged(), n=n)
    assert "negative table length" in call(*staged(), nseg=-1)
    for field, value in (("h", 0), ("w", 0), ("h", 16385), ("w", 16385)):
        assert "size outside" in call(*staged(**{f"m__{field}__0": value}))
    assert "negative mask offset" in call(*staged(m__mask_offset__0=-4))
    assert "segment range" in call(*staged(m__seg_first__0=-1))
    assert "segment range" in call(*staged(m__seg_count__0=3))
    assert "segment range" in call(*staged(m__seg_first__0=1, m__seg_count__0=2))
    assert "segment range" in call(*staged(), nseg=1)
    assert "toggle offset" in call(*staged(s__toggle_offset__0=-4))
    assert "toggle offset" in call(*staged(s__toggle_offset__1=90))      # misaligned
    assert "negative toggle count" in call(*staged(s__count__0=-1))
    for field, row, value in (("col_first", 0, -1), ("col_last", 0, w), ("col_first", 1, 7), ("col_last", 1, 7)):
        assert "column range outside" in call(*staged(**{f"s__{field}__{row}": value}))
    assert "does not hold" in call(*staged(s__col_first__0=1))           # the first toggle lies in column 0
    assert "does not hold" in call(*staged(s__col_last__0=3))            # covered through pixel 29: column 4
    assert "does not hold" in call(*staged(s__col_last__1=5))            # an odd count covers through the last column
    buf, md, sd = stage_one(cm, good, h, w)
    tog = buf[int(sd["toggle_offset"][0]):][:16].view(np.uint32)
    tog[:] = [3, 9, 9, 30]
    assert "strictly increasing" in call(buf, md, sd)
    tog[:] = [3, 20, 9, 30]
    assert "strictly increasing" in call(buf, md, sd)
    tog[:] = [3, 9, 20, h * w + 1]
    assert "above h*w" in call(buf, md, sd)
    tog[:] = [3, 9, 20, h * w]                                            # a toggle at h*w is legal
    sd["col_last"][0] = w - 1
    rc = lib.hh_debug_crowd_masks_host(np.zeros(h * w, np.uint8).ctypes.data, md.ctypes.data, sd.ctypes.data, buf.ctypes.data, 2)
    assert rc == 0
    # the host walk refuses the same tables with its own name
    buf, md, sd = staged(m__h__0=0)
    assert lib.hh_debug_crowd_masks_host(np.zeros(64, np.uint8).ctypes.data, md.ctypes.data, sd.ctypes.data, buf.ctypes.data, 2) == 1
    assert lib.hh_last_error().decode().startswith("hh_debug_crowd_masks_host: ")


def test_crowd_segments_object(cm):
    s = cm.CrowdSegments(6, 7, [[3, 9], [], np.array([1], np.uint32), [42]])
    assert s.shape == (6, 7) and len(s.toggle_lists) == 3 and all(t.dtype == np.uint32 for t in s.toggle_lists)
    assert s.table_bytes == 24 + 3 * 24 + 4 * 4
    assert [s.column_range(t) for t in s.toggle_lists] == [column_range(t, 6, 7) for t in s.toggle_lists] == [(0, 1), (0, 6), (6, 6)]
    for bad in ([[9, 3]], [[3, 3]], [[43]], [[-1, 4]]):
        with pytest.raises(ValueError):
            cm.CrowdSegments(6, 7, bad)
    for h, w in ((0, 7), (6, 16385)):
        with pytest.raises(ValueError):
            cm.CrowdSegments(h, w)


def test_annotation_dispatch(cm):
    h, w = 12, 14
    rle = {"counts": [10, 20, 138], "size": [h, w]}
    tri, quad, box = [1.5, 1.2, 9.3, 2.0, 4.1, 10.7], [2, 2, 2, 9, 8, 9, 8, 2], [3, 4, 5, 6]
    annot = [person(1, 0, rle), person(0, 0, [tri, quad], 1), person(0, 5, [[0, 0, 0, 11, 13, 11, 13, 0]], 2), person(0, 0, [box, [1, 1, 2, 2]], 3),
             person(1, 3, [tri], 4)]
    s = cm.CrowdSegments.from_annotations(annot, h, w)
    want = [ref.rle_toggles(rle["counts"], h, w), ref.polygon_toggles(tri, h, w), ref.polygon_toggles(quad, h, w),
            ref.polygon_toggles([3, 4, 3, 10, 8, 10, 8, 4], h, w), ref.polygon_toggles([1, 1, 1, 3, 3, 3, 3, 1], h, w), ref.polygon_toggles(tri, h, w)]
    assert len(s.toggle_lists) == len(want) and all(np.array_equal(a, b) for a, b in zip(s.toggle_lists, want))
    assert all(np.array_equal(a, b) for a, b in zip(s.toggle_lists, ref.annotation_toggles(annot, h, w)))
    # the object with keypoints that is no crowd contributes nothing, although its polygon covers the whole image
    assert ref.crowd_mask_reference(annot, h, w).any()
    assert cm.CrowdSegments.from_annotations([annot[2]], h, w).toggle_lists == []
    # the dispatch looks at the FIRST entry only: a 4-number entry behind a polygon is a bad polygon, a polygon behind a box a bad box
    for bad in ([tri, box], [box, tri], [[1, 2, 3, 4, 5, 6, 7]], [[1, 2, 3, 4, 5]], [[1, 2]], [1, 2, 3, 4]):
        with pytest.raises(ValueError):
            cm.CrowdSegments.from_annotations([person(1, 0, bad)], h, w)
        with pytest.raises((ValueError, TypeError)):
            ref.annotation_toggles([person(1, 0, bad)], h, w)
    with pytest.raises(ValueError):
        cm.CrowdSegments.from_annotations([person(1, 0, {"counts": "abc", "size": [h, w]})], h, w)


def test_union_not_xor(pkg, cm):
    h, w = 10, 12
    a, b = [1, 1, 1, 7, 7, 7, 7, 1], [4, 3, 4, 9, 10, 9, 10, 3]
    lists = [ref.polygon_toggles(a, h, w), ref.polygon_toggles(b, h, w)]
    both = ref.covered(lists[0], h, w) & ref.covered(lists[1], h, w)
    assert both.sum() == 12
    rc, got = host_walk(pkg, lists, h, w)
    assert rc == 0 and (got[both] == 0).all() and np.array_equal(got, ref.mask_from_toggles(lists, h, w))
    assert ((got == 0) == (ref.covered(lists[0], h, w) | ref.covered(lists[1], h, w))).all()


def test_raw_sample(pkg, cm):
    h, w = 12, 14
    img = np.zeros((h, w, 3), np.uint8)
    annot = [person(0, 4, [[1, 1, 1, 5, 5, 5]], 0), person(1, 0, {"counts": [10, 20, 138], "size": [h, w]}, 1), person(1, 2, [[2, 2, 2, 9, 8, 9]], 2),
             person(0, 0, [[3, 4, 5, 6]], 3)]
    image, segs, joints = pkg.keypoints.raw_sample(img, annot)
    assert image is img and isinstance(segs, cm.CrowdSegments) and segs.shape == (h, w) and len(segs.toggle_lists) == 3
    # coco.py:464-465: iscrowd == 0 or num_keypoints > 0 -> objects 0, 2 and 3, in order
    assert joints.shape == (3, 17, 3) and joints.dtype == np.float64
    for row, i in zip(joints, (0, 2, 3)):
        assert np.array_equal(row, np.array(annot[i]["keypoints"]).reshape(-1, 3))
    assert pkg.keypoints.raw_sample(img, [])[2].shape == (0, 17, 3)
