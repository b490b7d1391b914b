"""-m gpu: hh_multi_scale_aggregate against the composition it replaces (bit for bit), and the batched multi-scale route of
InferenceKeypointsModel.infer_images / evaluate_images against the per-image call_multi_scale."""
import importlib

import numpy as np
import pytest
import torch

from conftest import PKG
from oracle import decode as orc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SCALES = (0.5, 1.0, 2.0)
RAW_SHAPES = [(150, 220), (220, 150), (150, 220), (128, 128), (150, 220), (150, 220)]
FIELDS = ("kpts_coords", "kpts_scores", "kpts_tags", "obj_scores")


@pytest.fixture(scope="module")
def nets(pkg):
    """Seeded synthetic nets, one per width for the whole module (building one costs more than the tests that use it)."""
    cache = {}

    def get(C):
        if C not in cache:
            net = pkg.HigherHRNet(17, C)
            net.load_state_dict({k: torch.from_numpy(pkg.synth.synth_param(k, v.shape, 3)) for k, v in net.state_dict().items()})
            cache[C] = net.to(DEV).eval()
        return cache[C]
    return get


@pytest.fixture(scope="module")
def images():
    rs = np.random.RandomState(9)
    return [rs.randint(0, 255, s + (3,)).astype(np.uint8) for s in RAW_SHAPES]


def _aggregate(pkg, srcs, perm, weights, dst, K):
    """srcs: [(hm tensor [B,>=K,h,w], flipped tensor or None)]; dst: a [B,K,H,W] view whose planes are contiguous."""
    S = pkg.keypoints.model._ScaleSrc
    table = (S * len(srcs))()
    for i, ((hm, hmf), wgt) in enumerate(zip(srcs, weights)):
        table[i] = S(hm.data_ptr(), hm.stride(0), None if hmf is None else hmf.data_ptr(), 0 if hmf is None else hmf.stride(0),
                     hm.shape[2], hm.shape[3], wgt)
    p = np.asarray(perm, np.int32)
    pkg._lib.check(pkg._lib.load().hh_multi_scale_aggregate(table, len(srcs), p.ctypes.data, dst.shape[0], K, dst.data_ptr(), dst.stride(0),
                                                           dst.shape[2], dst.shape[3], torch.cuda.current_stream().cuda_stream))


def _reference(srcs, perm, weights, K, H, W):
    """numpy flip merge, oracle bilinear per image, weight and sum rounded to fp32 one by one, in order."""
    acc = None
    for (hm, hmf), wgt in zip(srcs, weights):
        a = hm[:, :K]
        if hmf is not None:
            a = ((a + hmf[:, :K][:, perm][..., ::-1]) / np.float32(2)).astype(np.float32)
        r = np.stack([orc.bilinear(np.ascontiguousarray(a[b]), H, W) for b in range(a.shape[0])])
        v = (np.float32(wgt) * r).astype(np.float32)
        acc = v if acc is None else (acc + v).astype(np.float32)
    return acc


@pytest.mark.parametrize("K,perm", [(5, [0, 2, 1, 4, 3]), (17, None)])
def test_aggregate_equals_the_composed_cpu_reference(pkg, K, perm):
    """x2, identity, x0.5 and a non-integer ratio with an odd width under the flip; sources and dst are channel slices of wider
    tensors (batch strides beyond K planes); dst starts as NaN, its neighbours as 7.0."""
    perm = perm if perm is not None else list(pkg.keypoints.transforms_utils.COCO_FLIP_INDEX)
    B, H, W = 3, 16, 24
    rs = np.random.RandomState(11 + K)
    spec = [((8, 12), True), ((16, 24), False), ((32, 48), True), ((7, 9), True)]
    host = []
    for (h, w), flipped in spec:
        host.append((rs.randn(B, 2 * K, h, w).astype(np.float32), rs.randn(B, 2 * K, h, w).astype(np.float32) if flipped else None))
    dev = [(torch.from_numpy(a).to(DEV), None if f is None else torch.from_numpy(f).to(DEV)) for a, f in host]
    for pick in ([0, 1, 2, 3], [0], [0, 1, 2, 3, 3, 2, 1, 0]):  # nsrc = 4, 1, 8
        wgt = 1.0 / 4 if len(pick) == 4 else 1.0 / len(pick)
        weights = [wgt] * len(pick)
        full = torch.empty((B, K + 2, H, W), device=DEV)
        full[:, :K] = float("nan")
        full[:, K:] = 7.0
        _aggregate(pkg, [dev[i] for i in pick], perm, weights, full[:, :K], K)
        got = full.cpu().numpy()
        assert not np.isnan(got).any() and (got[:, K:] == 7.0).all()
        ref = _reference([host[i] for i in pick], perm, weights, K, H, W)
        assert np.array_equal(got[:, :K], ref), (len(pick), int((got[:, :K] != ref).sum()))


def test_aggregate_equals_flip_merge_and_resize_accumulate(pkg):
    """The launch against the entry points it stands for, on a dst whose W is no multiple of 4 (scalar stores and tails)."""
    lib = pkg._lib.load()
    B, K, H, W = 2, 17, 40, 54
    perm = np.asarray(pkg.keypoints.transforms_utils.COCO_FLIP_INDEX, np.int32)
    g = torch.Generator().manual_seed(5)
    srcs = []
    for (h, w), flipped in [((20, 27), True), ((40, 54), False), ((80, 108), True)]:
        srcs.append((torch.randn((B, K, h, w), generator=g).to(DEV), torch.randn((B, K, h, w), generator=g).to(DEV) if flipped else None))
    wgt = 1.0 / 3
    got = torch.full((B, K, H, W), float("nan"), device=DEV)
    _aggregate(pkg, srcs, perm, [wgt] * 3, got, K)
    st = torch.cuda.current_stream().cuda_stream
    ref = torch.full((B, K, H, W), float("nan"), device=DEV)
    for i, (hm, hmf) in enumerate(srcs):
        m = hm.clone()
        if hmf is not None:
            pkg._lib.check(lib.hh_flip_merge(m.data_ptr(), m.stride(0), hmf.data_ptr(), hmf.stride(0), None, 0, None, 0, perm.ctypes.data, B, K,
                                             m.shape[2], m.shape[3], st))
        pkg._lib.check(lib.hh_resize_accumulate(m.data_ptr(), m.stride(0), B, K, m.shape[2], m.shape[3], ref.data_ptr(), ref.stride(0), H, W,
                                                wgt, int(i == 0), st))
    assert not got.isnan().any() and torch.equal(got, ref)


def _same_result(a, b):
    for f in FIELDS:
        x, y = getattr(a, f), getattr(b, f)
        assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y), f


@pytest.mark.parametrize("use_flip", [False, True])
@pytest.mark.parametrize("C", [32, 48])
def test_infer_images_multi_scale_equals_call_multi_scale(pkg, nets, images, C, use_flip):
    """One bucket of four that splits 3 + 1, two buckets of one, scale-2 sub-batches of one image: every image gets what
    call_multi_scale returns for it, bit for bit."""
    model = pkg.InferenceKeypointsModel(nets(C), det_thr=0.05, tag_thr=0.5, use_flip=use_flip, input_size=128, device=DEV)
    batched = model.infer_images(images, max_batch=3, scales=SCALES)
    assert len(batched) == len(images)
    for im, rb in zip(images, batched):
        r1 = model.call_multi_scale(im, None, SCALES)
        assert rb.raw_image is im
        _same_result(rb, r1)
        assert torch.equal(rb.model_input_image, r1.model_input_image)


@pytest.mark.parametrize("use_flip", [False, True])
def test_single_scale_through_the_aggregation_equals_the_plain_batched_path(pkg, nets, images, use_flip):
    """scales=(1.0,): ratio 1 makes the interpolation weights exactly 1 and 0 and the weight is 1, so the aggregated maps are the
    scale-1 maps."""
    model = pkg.InferenceKeypointsModel(nets(32), det_thr=0.05, tag_thr=0.5, use_flip=use_flip, input_size=128, device=DEV)
    for ra, rb in zip(model.infer_images(images, max_batch=3, scales=(1.0,)), model.infer_images(images, max_batch=3)):
        _same_result(ra, rb)


def test_evaluate_images_multi_scale_batched_equals_per_image(pkg, nets, images):
    ev = importlib.import_module(PKG + ".keypoints.evaluation")
    model = pkg.InferenceKeypointsModel(nets(32), det_thr=0.05, tag_thr=0.5, use_flip=True, input_size=128, device=DEV)
    ids = list(range(21, 21 + len(images)))
    batched = ev.evaluate_images(model, images, ids, multi_scale=SCALES, batch=3)
    assert batched == ev.evaluate_images(model, images, ids, multi_scale=SCALES, batch=1) and len(batched) >= len(images)
