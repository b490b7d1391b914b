"""Batched multi-scale test, the parts that need no GPU: the host planner (plan_multi_scale) against the oracle's size arithmetic
and its own covering / pixel-budget rules, and the argument checks of hh_multi_scale_aggregate, which all come before the entry's
first HIP call."""
import ctypes as C
import importlib
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, PKG
from oracle import transforms as ot

SCALES = (0.5, 1.0, 2.0)
GPU_TEST_SHAPES = [(150, 220), (220, 150), (150, 220), (128, 128), (150, 220), (150, 220)]  # tests/test_gpu_multi_scale.py


@pytest.fixture(scope="module")
def km(pkg):
    return importlib.import_module(PKG + ".keypoints.model")


def _golden_rows():
    return json.load(open(os.path.join(GOLDEN, "multi_scale_size.json")))


def test_plan_sizes_equal_the_oracle(km):
    for r in _golden_rows():
        plan = km.plan_multi_scale([(r["h"], r["w"])], r["input_size"], SCALES, 32)
        assert len(plan) == 1 and plan[0]["images"] == [0]
        for si, s in enumerate(SCALES):
            assert tuple(plan[0]["sizes"][si]) == tuple(ot.get_multi_scale_size((r["h"], r["w"]), r["input_size"], s, min(SCALES))[0])


@pytest.mark.parametrize("max_batch", [1, 3, 32])
@pytest.mark.parametrize("input_size", [128, 512, 640])
def test_plan_covers_every_image_once_within_the_pixel_budget(km, max_batch, input_size):
    shapes = GPU_TEST_SHAPES + [(r["h"], r["w"]) for r in _golden_rows()]
    plan = km.plan_multi_scale(shapes, input_size, SCALES, max_batch)
    seen = [i for c in plan for i in c["images"]]
    assert sorted(seen) == list(range(len(shapes))) and len(seen) == len(shapes)
    i1 = SCALES.index(1.0)
    for c in plan:
        n = len(c["images"])
        assert 1 <= n <= max_batch and c["images"] == sorted(c["images"])
        assert len(c["sizes"]) == len(c["sub_batches"]) == len(SCALES)
        for i in c["images"]:  # one bucket = the same model-input size at EVERY scale
            for si, s in enumerate(SCALES):
                assert tuple(c["sizes"][si]) == tuple(ot.get_multi_scale_size(shapes[i], input_size, s, min(SCALES))[0])
        w1, h1 = c["sizes"][i1]
        for (ws, hs), subs in zip(c["sizes"], c["sub_batches"]):
            # consecutive ranges that cover 0..n once, in order
            assert subs[0][0] == 0 and subs[-1][1] == n
            assert all(lo < hi for lo, hi in subs) and all(a[1] == b[0] for a, b in zip(subs[:-1], subs[1:]))
            n_s = max(hi - lo for lo, hi in subs)
            assert n_s == min(n, max(1, max_batch * h1 * w1 // (hs * ws)))
            assert all(hi - lo == n_s for lo, hi in subs[:-1])
            assert n_s * hs * ws <= max_batch * h1 * w1 or n_s == 1
        assert c["sub_batches"][i1] == [(0, n)]  # the scale-1 pass (tags, geometry) is one forward per chunk


def test_plan_of_the_gpu_test_images(km):
    """input_size 128, max_batch 3: one bucket of four that splits 3 + 1, scale-2 sub-batches of one image."""
    plan = km.plan_multi_scale(GPU_TEST_SHAPES, 128, SCALES, 3)
    assert [c["images"] for c in plan] == [[0, 2, 4], [5], [1], [3]]
    assert plan[0]["sizes"] == ((128, 64), (256, 128), (512, 256))
    assert plan[0]["sub_batches"] == [[(0, 3)], [(0, 3)], [(0, 1), (1, 2), (2, 3)]]


def test_plan_needs_scale_one(km):
    with pytest.raises(ValueError):
        km.plan_multi_scale([(480, 640)], 512, (0.5, 2.0), 8)
    with pytest.raises(ValueError):
        km.plan_multi_scale([(480, 640)], 512, (), 8)


def _call(pkg, srcs, nsrc, perm, B, K, dst, dst_bs, H, W, null_table=False):
    lib = pkg._lib.load()
    table = (pkg.keypoints.model._ScaleSrc * max(len(srcs), 1))()
    for i, (hm, bs, hmf, fbs, h, w) in enumerate(srcs):
        table[i] = pkg.keypoints.model._ScaleSrc(hm, bs, hmf, fbs, h, w, 0.5)
    p = None if perm is None else np.asarray(perm, np.int32)
    rc = lib.hh_multi_scale_aggregate(None if null_table else table, nsrc, None if p is None else p.ctypes.data, B, K, dst, dst_bs, H, W, None)
    return rc, lib.hh_last_error().decode()


def test_aggregate_refuses_bad_arguments_before_any_device_call(pkg):
    """No GPU here: every case must be turned away by the host checks (a call that got as far as the launch would fail differently,
    or crash on the made-up addresses)."""
    A = 0x1000  # a non-null address that is never dereferenced
    K, h, w, H, W = 17, 8, 12, 16, 24
    ok = (A, K * h * w, None, 0, h, w)
    okf = (A, K * h * w, A, K * h * w, h, w)
    perm = list(range(K))
    dbs = K * H * W
    cases = {
        "nsrc 0": dict(srcs=[ok], nsrc=0),
        "nsrc 9": dict(srcs=[ok] * 9, nsrc=9),
        "null srcs_host": dict(srcs=[ok], null_table=True),
        "null dst": dict(srcs=[ok], dst=None),
        "null hm": dict(srcs=[ok, (None, K * h * w, None, 0, h, w)]),
        "null perm with a flipped source": dict(srcs=[ok, okf], perm=None),
        "K 0": dict(srcs=[ok], K=0),
        "K 65": dict(srcs=[(A, 65 * h * w, None, 0, h, w)], K=65, dst_bs=65 * H * W, perm=list(range(65))),
        "B 0": dict(srcs=[ok], B=0),
        "H 0": dict(srcs=[ok], H=0),
        "W -1": dict(srcs=[ok], W=-1),
        "source h 0": dict(srcs=[(A, K * h * w, None, 0, 0, w)]),
        "source w 0": dict(srcs=[(A, K * h * w, None, 0, h, 0)]),
        "dst_bstride short": dict(srcs=[ok], dst_bs=dbs - 1),
        "source bstride short": dict(srcs=[(A, K * h * w - 1, None, 0, h, w)]),
        "flipped bstride short": dict(srcs=[(A, K * h * w, A, K * h * w - 1, h, w)]),
    }
    for name, kw in cases.items():
        a = dict(srcs=[ok], perm=perm, B=2, K=K, dst=A, dst_bs=dbs, H=H, W=W, null_table=False)
        a.update(kw)
        a.setdefault("nsrc", len(a["srcs"]))
        rc, msg = _call(pkg, a["srcs"], a["nsrc"], a["perm"], a["B"], a["K"], a["dst"], a["dst_bs"], a["H"], a["W"], a["null_table"])
        assert rc != 0 and msg.startswith("hh_multi_scale_aggregate:"), (name, rc, msg)


def test_scale_src_struct_matches_the_header(pkg):
    """hh_scale_src of include/hhrnet.h as the binding lays it out: 48 bytes, the offsets of a C compiler on this ABI."""
    S = pkg.keypoints.model._ScaleSrc
    assert C.sizeof(S) == 48
    assert [getattr(S, f).offset for f, _ in S._fields_] == [0, 8, 16, 24, 32, 36, 40]
