"""Crowd masks filled on the device (hh_crowd_masks_u8_batch, keypoints/crowd_mask.py) against the numpy restatement of the rule
(tests/crowd_mask_ref.py), byte for byte, at the smallest shapes where the kernel can go wrong, and TrainInput.build from CrowdSegments
against the same build from the dense masks of crowd_mask_reference.  Everything here is an equality of bits."""
import numpy as np
import pytest
import torch

import crowd_mask_ref as ref
from crowd_mask_helpers import BOW_TIE, OFF_BOTTOM, OFF_LEFT, OFF_RIGHT, OFF_TOP, TRIANGLE, cm, person  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 0x5B  # neither 0 nor 255: an unwritten mask byte shows, and so does a write outside a mask


def fill(cm, items, residues=(0, 1, 2, 3), gap=5):  # noqa: F811
    """hh_crowd_masks_u8_batch through the module's own staging, all `items` in ONE launch, mask i at an offset with residue
    residues[i % len] mod 4 and `gap`..`gap + 3` guard bytes in front of it, into a buffer prefilled with SENTINEL
    -> ([uint8 [h,w]], were all bytes outside the masks left alone)."""
    staged = (cm.tables_bytes(items) + 63) // 64 * 64
    at, offs = staged, []
    for i, s in enumerate(items):
        at += gap
        at += (residues[i % len(residues)] - at) % 4
        offs.append(at)
        at += s.h * s.w
    total = at + gap
    host = torch.full((total,), SENTINEL, dtype=torch.uint8)
    desc_at, seg_at, nseg = cm.fill_tables(items, offs, host.numpy(), 0)
    dev = torch.device(DEV)
    raw = host.to(dev)
    cm.launch(dev, raw.data_ptr(), host.data_ptr(), desc_at, seg_at, len(items), nseg)
    back = raw.cpu().numpy()
    outside = np.ones(total, bool)
    outside[:staged] = False
    masks = []
    for s, o in zip(items, offs):
        masks.append(back[o:o + s.h * s.w].reshape(s.h, s.w).copy())
        outside[o:o + s.h * s.w] = False
    assert np.array_equal(back[:staged], host.numpy()[:staged])  # the tables are read, never written
    return masks, bool((back[outside] == SENTINEL).all())


def random_lists(rng, h, w, segments, toggles):
    return [np.unique(rng.randint(0, h * w + 1, toggles)).astype(np.uint32) for _ in range(segments)]


@pytest.fixture(scope="module")
def kernel_cases(cm):  # noqa: F811
    """[(tag, CrowdSegments)]: built once."""
    th, tw, _, chunk = cm.config()
    rng = np.random.RandomState(11)
    cases = [("1x1 covered", cm.CrowdSegments(1, 1, [[0]])), ("1x1 free", cm.CrowdSegments(1, 1, [[1]])), ("1x1 no segment", cm.CrowdSegments(1, 1)),
             ("1xN", cm.CrowdSegments(1, tw + 7, random_lists(rng, 1, tw + 7, 2, 30))), ("Nx1", cm.CrowdSegments(2 * th + 5, 1, random_lists(rng, 2 * th + 5, 1, 2, 9))),
             ("no segment", cm.CrowdSegments(th + 3, 21))]
    for h in (th - 1, th, th + 1):
        for w in (tw - 1, tw, tw + 1):
            cases.append((f"tile {h}x{w}", cm.CrowdSegments(h, w, random_lists(rng, h, w, 3, 60))))
    for w in (5, 6, 7, 2 * tw + 2):  # no multiple of 4
        cases.append((f"ragged w={w}", cm.CrowdSegments(th + 2, w, random_lists(rng, th + 2, w, 2, 25))))
    h, w = 40, 45
    sides = [OFF_LEFT, OFF_RIGHT, OFF_TOP, OFF_BOTTOM]
    scaled = [[v * 5 for v in xy] for xy in sides]  # the h = 8, w = 9 fixtures blown up to 40 x 45: each leaves one side
    cases.append(("four sides", cm.CrowdSegments(h, w, [ref.polygon_toggles(xy, h, w) for xy in scaled])))
    overlap = [[v * 4 for v in TRIANGLE], [v * 4 for v in BOW_TIE], [3, 3, 3, 30, 30, 30, 30, 3], [10, 10, 10, 39, 44, 39, 44, 10]]
    cases.append(("overlapping", cm.CrowdSegments(h, w, [ref.polygon_toggles(xy, h, w) for xy in overlap])))
    cases.append(("toggle at h*w", cm.CrowdSegments(7, 9, [[5, 63], [63], [60]])))
    # more toggles in one segment than any per-chunk capacity: every pixel of a two-tile-wide mask toggles (and twice the capacity)
    h, w = th + 1, 2 * tw + 1
    many = np.arange(0, h * w + 1, dtype=np.uint32)
    assert many.size > 2 * max(chunk, 1)
    cases.append(("dense toggles", cm.CrowdSegments(h, w, [many, many[1::3]])))
    return cases


def test_kernel_equals_restatement_in_one_launch(cm, kernel_cases):  # noqa: F811
    items = [s for _, s in kernel_cases]
    got, clean = fill(cm, items)
    for (tag, s), g in zip(kernel_cases, got):
        want = ref.mask_from_toggles(s.toggle_lists, s.h, s.w)
        assert np.array_equal(g, want), f"{tag}: {int((g != want).sum())} of {want.size} bytes differ"
    assert clean, "a byte outside the masks was written"
    tags = dict(kernel_cases)
    assert (got[items.index(tags["no segment"])] == 255).all()
    four = got[items.index(tags["four sides"])] == 0
    assert four[:, 0].any() and four[:, -1].any() and four[0].any() and four[-1].any()


@pytest.mark.parametrize("residue", [0, 1, 2, 3])
def test_every_offset_residue(cm, kernel_cases, residue):  # noqa: F811
    """Each mask shape at each residue of its offset mod 4 (dword and byte stores change places with it)."""
    picked = [s for tag, s in kernel_cases if tag.startswith(("tile", "ragged", "1xN", "dense"))]
    got, clean = fill(cm, picked, residues=(residue,), gap=4)
    for s, g in zip(picked, got):
        assert np.array_equal(g, ref.mask_from_toggles(s.toggle_lists, s.h, s.w)), (s.shape, residue)
    assert clean


def annotation(h, w, seed):
    """A COCO annotation with a crowd run-length object, an unlabelled person with two polygons, a box object and labelled people."""
    rng = np.random.RandomState(seed)
    runs = rng.randint(0, max(h * w // 8, 1), 7)
    runs = runs.tolist() + [h * w - int(runs.sum())]
    poly = lambda k: (rng.uniform(-3, [w + 3, h + 3], (k, 2))).reshape(-1).tolist()  # noqa: E731
    return [person(0, 5, [poly(5)], seed), person(1, 0, {"counts": runs, "size": [h, w]}, seed + 1), person(0, 0, [poly(4), poly(7)], seed + 2),
            person(0, 0, [[w // 3, h // 4, w // 5, h // 3]], seed + 3), person(1, 2, [poly(6)], seed + 4)]


def test_crowd_masks_and_get_crowd_mask_round_trip(pkg, cm):  # noqa: F811
    sizes = [(37, 53), (64, 80), (1, 1), (50, 300)]
    annots = [annotation(h, w, 40 + i) for i, (h, w) in enumerate(sizes)] + [[]]
    sizes.append((9, 11))
    segs = [cm.CrowdSegments.from_annotations(a, h, w) for a, (h, w) in zip(annots, sizes)]
    old, cm.CHUNK_BYTES = cm.CHUNK_BYTES, 6000  # several chunks: [0], [1, 2], [3], [4]
    try:
        chunked = pkg.keypoints.crowd_masks(segs, DEV)
    finally:
        cm.CHUNK_BYTES = old
    whole = pkg.keypoints.crowd_masks(segs, DEV)
    for a, (h, w), c, g in zip(annots, sizes, chunked, whole):
        want = ref.crowd_mask_reference(a, h, w)
        assert g.dtype == np.bool_ and g.shape == (h, w) and np.array_equal(g, want) and np.array_equal(c, want)
    assert whole[-1].all() and not whole[1].all()
    assert np.array_equal(pkg.keypoints.get_crowd_mask(annots[0], *sizes[0], device=DEV), ref.crowd_mask_reference(annots[0], *sizes[0]))
    assert pkg.keypoints.crowd_masks([], DEV) == []


def raw_pair(pkg, h, w, seed, crowded=True):
    """The same raw sample twice: with CrowdSegments (keypoints.raw_sample) and with the dense mask of the restatement."""
    rng = np.random.RandomState(seed)
    img = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
    annot = annotation(h, w, seed) if crowded else [person(0, 6, [[1, 1, 1, 9, 9, 9]], seed)]
    image, segs, joints = pkg.keypoints.raw_sample(img, annot)
    return (image, segs, joints), (image, ref.crowd_mask_reference(annot, h, w), joints)


def assert_same_batch(a, b):
    assert torch.equal(a[0], b[0])
    for k in (1, 2):
        assert len(a[k]) == len(b[k]) and all(torch.equal(x, y) for x, y in zip(a[k], b[k]))
    assert all(torch.equal(x.packed, y.packed) and torch.equal(x.counts, y.counts) and x.geometry == y.geometry for x, y in zip(a[3], b[3]))


@pytest.mark.parametrize("kind", ["plain", "mosaic"])
def test_train_input_from_segments_equals_dense(pkg, cm, kind):  # noqa: F811
    ti_mod = pkg.keypoints.train_input
    S = 64
    ti = ti_mod.TrainInput(S, [1 / 4, 1 / 2], device=DEV)
    # every h * w is a multiple of 64: no padding differs between the two layouts, so the byte counts can be compared exactly
    pairs = [raw_pair(pkg, 64, 80, 1), raw_pair(pkg, 48, 64, 2, crowded=False), raw_pair(pkg, 56, 72, 3), raw_pair(pkg, 40, 48, 4), raw_pair(pkg, 128, 128, 5)]
    param = lambda h, w, i: ti_mod.AugParams(min(h, w) / 200 * (0.8 + 0.2 * i), 25.0 * i - 30, (w / 2 + 3 * i, h / 2 - 2 * i), bool(i % 2))  # noqa: E731
    if kind == "plain":
        seg_batch, dense_batch = [p[0] for p in pairs[:3]], [p[1] for p in pairs[:3]]
        params = [param(*s[0].shape[:2], i) for i, s in enumerate(seg_batch)]
        travelling = pairs[:3]
    else:
        seg_batch = [ti_mod.Mosaic([p[0] for p in pairs[:4]]), pairs[4][0], ti_mod.Mosaic([pairs[i][0] for i in (4, 2, 2, 0)])]
        dense_batch = [ti_mod.Mosaic([p[1] for p in pairs[:4]]), pairs[4][1], ti_mod.Mosaic([pairs[i][1] for i in (4, 2, 2, 0)])]
        params = [param(2 * S, 2 * S, 1), param(128, 128, 2), param(2 * S, 2 * S, 3)]
        travelling = pairs[:4] + [pairs[4]] + [pairs[i] for i in (4, 2, 2, 0)]
    dense = ti.build(dense_batch, params)
    dense_bytes, dense_launches = ti.last_h2d_bytes, ti.last_launches
    segs = ti.build(seg_batch, params)
    seg_bytes, seg_launches = ti.last_h2d_bytes, ti.last_launches
    assert_same_batch(segs, dense)
    assert all(0 < float(m.mean()) < 1 for m in dense[2]), "the crowd masks of this batch are trivial"
    mask_bytes = sum(p[0][1].h * p[0][1].w for p in travelling)
    table_bytes = sum(p[0][1].table_bytes for p in travelling)
    assert table_bytes == sum(24 + 24 * len(p[0][1].toggle_lists) + 4 * sum(t.size for t in p[0][1].toggle_lists) for p in travelling)
    assert dense_bytes - seg_bytes == mask_bytes - table_bytes and mask_bytes > table_bytes
    assert seg_launches == dense_launches + 1
    # dense and segment samples mixed in one batch
    mixed = [d if i % 2 else s for i, (s, d) in enumerate(zip(seg_batch, dense_batch))]
    assert_same_batch(ti.build(mixed, params), dense)
    assert ti.last_launches == dense_launches + 1
    if kind == "mosaic":  # ... and mixed among the tiles of one mosaic
        tiles = lambda m: [d if j % 2 else s for j, (s, d) in enumerate(zip(seg_batch[m].tiles, dense_batch[m].tiles))]  # noqa: E731
        assert_same_batch(ti.build([ti_mod.Mosaic(tiles(0)), dense_batch[1], ti_mod.Mosaic(tiles(2))], params), dense)
        assert ti.last_launches == dense_launches + 1
    again =ti.build(dense_batch, params)  # the dense path is what it was: same bytes, same launches
    assert_same_batch(again, dense)
    assert (ti.last_h2d_bytes, ti.last_launches) == (dense_bytes, dense_launches)
