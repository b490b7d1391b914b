"""The training input built on the device (keypoints/train_input.py over hh_train_images_u8_batch, hh_train_masks_u8_batch and
hh_render_heatmaps): bit-identical to the reference-run golden, to oracle.transforms.warp_affine on a lattice of augmentations at
512^2, and to targets.HeatmapGenerator over map sizes, sigmas and joint placements.  Everything here is an equality of bits: the
warps are integer arithmetic, the heatmaps a maximum over fp32 table entries, the normalisation the three fp32 operations of
preprocess_pixel in its order."""
import hashlib
import importlib

import numpy as np
import pytest
import torch

from conftest import PKG
from oracle import transforms as otf
from train_input_helpers import golden, golden_draw, golden_sample, golden_transform, ti_mod  # noqa: F401  (fixtures + helpers)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def normalized(u8_hwc, mean, std):
    """Normalize(ToTensor(u8)) as preprocess_pixel forms it: ((float)v / 255.0f - mean) / std, all fp32 -> [3,H,W]."""
    x = u8_hwc.astype(np.float32).transpose(2, 0, 1) / np.float32(255)
    return (x - np.asarray(mean, np.float32)[:, None, None]) / np.asarray(std, np.float32)[:, None, None]


def oracle_sample(ti, sample, p):
    """One sample through the reference's definition with oracle.transforms.warp_affine as the warp:
    -> (uint8 image [S,S,3], [mask fp32 [s,s]], [int joints])."""
    img, mask, joints = sample
    mat_image, mats, _, ints = ti.geometry(img.shape[0], img.shape[1], joints, p)
    out = otf.warp_affine(img, mat_image, (ti.out_size, ti.out_size))
    masks = [(otf.warp_affine((mask * 255).astype(np.uint8), m, (s, s)) / 255 > 0.5).astype(np.float32) for m, s in zip(mats, ti.hm_sizes)]
    if p.flip:
        out, masks = out[:, ::-1], [m[:, ::-1] for m in masks]
    return np.ascontiguousarray(out), [np.ascontiguousarray(m) for m in masks], ints


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def test_golden_cases_bit_identical(pkg, ti_mod, golden):  # noqa: F811
    """Images, masks, heatmaps and packed joints of every golden case, each mode's cases as ONE batch of mixed raw sizes."""
    meta, data = golden
    loss = importlib.import_module(PKG + ".keypoints.loss")
    for mode_name in ("train", "train_long", "inference"):
        cases = [c for c in meta["cases"] if c["mode"] == mode_name]
        ti, mode = golden_transform(ti_mod, meta, cases[0], device=DEV)
        samples = [golden_sample(pkg, meta, c) for c in cases]
        params = [golden_draw(mode, c)[0] for c in cases]
        images, heatmaps, masks, joints = ti.build(samples, params)
        torch.cuda.synchronize()
        for b, c in enumerate(cases):
            tag = c["tag"]
            u8 = data[f"{tag}.image_u8"] if f"{tag}.image_u8" in data else oracle_sample(ti, samples[b], params[b])[0]
            assert hashlib.sha256(u8.tobytes()).hexdigest() == c["image_sha256"], tag  # (the fixture-time image, stored or recomputed)
            assert same_bits(images[b].cpu().numpy(), normalized(u8, ti.mean, ti.std)), tag
            for i in range(len(ti.hm_sizes)):
                assert same_bits(masks[i][b].cpu().numpy(), data[f"{tag}.mask{i}"].astype(np.float32)), (tag, i)
                assert same_bits(heatmaps[i][b].cpu().numpy(), data[f"{tag}.hm{i}"]), (tag, i)
        for i, s in enumerate(ti.hm_sizes):
            packed, counts = loss.pack_joints([data[f"{c['tag']}.joints_i{i}"] for c in cases], meta["num_kpts"], s, s)
            assert same_bits(joints[i].packed.cpu().numpy(), packed) and same_bits(joints[i].counts.cpu().numpy(), counts)


def test_warp_lattice_512_against_the_oracle(pkg, ti_mod):  # noqa: F811
    """Rotation +-30 degrees x scale 0.75 / 1.5 x the translate extremes x flip, sources smaller and larger than the 512^2 output,
    all-true / all-false / holed masks: image, both stages' masks bit for bit against oracle.transforms.warp_affine."""
    ti = ti_mod.TrainInput(512, [1 / 4, 1 / 2], device=DEV)
    samples, params = [], []
    idx = 0
    for rot in (-30.0, 30.0):
        for aug_scale in (0.75, 1.5):
            for sign in (-1, 1):
                for flip in (False, True):
                    h, w = ((300, 400), (700, 900))[(idx // 2 + idx) % 2]
                    samples.append(pkg.synth.synth_train_sample(h, w, 3, 40 + idx, holes=(0, -1, 2)[idx % 3]))
                    scale = min(h, w) / 200 * aug_scale
                    reach = int(40 * scale)  # np.random.randint(-reach, reach): the extremes are -reach and reach - 1
                    shift = -reach if sign < 0 else reach - 1
                    params.append(ti_mod.AugParams(scale, rot, (w / 2 + shift, h / 2 + shift), flip))
                    idx += 1
    assert {s[0].shape[0] for s in samples} == {300, 700} and any(s[1].all() for s in samples) and any(not s[1].any() for s in samples)
    images, _, masks, _ = ti.build(samples, params)
    torch.cuda.synchronize()
    images, masks = images.cpu().numpy(), [m.cpu().numpy() for m in masks]
    for b, (s, p) in enumerate(zip(samples, params)):
        u8, ref_masks, _ = oracle_sample(ti, s, p)
        assert same_bits(images[b], normalized(u8, ti.mean, ti.std)), (b, p)
        for i in range(2):
            assert same_bits(masks[i][b], ref_masks[i]), (b, i, p)
    assert 0 < masks[1].mean() < 1


def render(pkg, joints, counts, table, reach, K, h, w):
    """hh_render_heatmaps through the C-ABI into a NaN-filled buffer (every element must be written)."""
    lib = pkg._lib.load()
    jd, cd, td = torch.from_numpy(joints).to(DEV), torch.from_numpy(counts).to(DEV), torch.from_numpy(table).to(DEV)
    out = torch.full((joints.shape[0], K, h, w), float("nan"), device=DEV, dtype=torch.float32)
    pkg._lib.check(lib.hh_render_heatmaps(jd.data_ptr(), cd.data_ptr(), joints.shape[0], joints.shape[1], K, td.data_ptr(), table.shape[0], reach,
                                          out.data_ptr(), h, w, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def render_case(h, w, K, seed):
    """-> joints int32 [3,32,K,3], counts: image 0 has no people, image 1 thirty (corners, coincident and overlapping bumps,
    invisible and out-of-map joints), image 2 four; every row beyond num_people holds VISIBLE in-map joints that must be ignored."""
    rs = np.random.RandomState(seed)
    B, P = 3, 32
    j = np.zeros((B, P, K, 3), np.int32)
    j[..., 0], j[..., 1], j[..., 2] = rs.randint(0, w, (B, P, K)), rs.randint(0, h, (B, P, K)), 1
    counts = np.array([0, 30, 4], np.int32)
    j[1, 0, :, :2] = (0, 0)                      # joints at 0 ...
    j[1, 1, :, 0], j[1, 1, :, 1] = w - 1, h - 1  # ... and at s - 1
    j[1, 2, :, 0], j[1, 2, :, 1] = 0, h - 1
    j[1, 3], j[1, 4] = j[1, 5], j[1, 5]          # coincident
    j[1, 6, :, :2] = j[1, 5, :, :2] + (1, -2)    # overlapping (may leave the map at a border: then it is an out-of-map joint)
    j[1, 7:12, :, 2] = rs.randint(-1, 2, (5, K))  # invisible (0) and negative visibility
    j[1, 12, :, 0], j[1, 13, :, 1], j[1, 14, :, 0] = w, -1, -5  # visible but outside the map
    return j, counts


@pytest.mark.parametrize("s", [32, 64, 128, 256])
@pytest.mark.parametrize("sigma", [1, 2, "s/64"])
def test_render_heatmaps_against_the_generator(pkg, ti_mod, s, sigma):  # noqa: F811
    K = 17
    sigma = s / 64 if sigma == "s/64" else sigma
    if 3 * sigma + 1 != int(3 * sigma + 1):  # s = 32: sigma 0.5 -- the accepted set is "3 sigma + 1 an integer": refused with a message
        with pytest.raises(pkg._lib.HHError, match="3 \\* sigma \\+ 1"):
            ti_mod.bump_table(sigma)
        return
    table, reach = ti_mod.bump_table(sigma)
    gen = pkg.keypoints.targets.HeatmapGenerator(K, s, sigma)
    joints, counts = render_case(s, s, K, seed=s + int(sigma))
    got = render(pkg, joints, counts, table, reach, K, s, s)
    for b in range(len(counts)):
        assert same_bits(got[b], gen(joints[b, :counts[b]])), (s, sigma, b)
    assert not got[0].any() and got[1].max() == 1.0


@pytest.mark.parametrize("h,w", [(48, 80), (40, 50), (7, 3), (20, 1028)])
def test_render_heatmaps_non_square(pkg, ti_mod, h, w):  # noqa: F811
    """Non-square maps, widths that are not multiples of 4 (scalar stores) and more than 256 groups a row (several items per thread), against
    the gather written out in numpy."""
    K, sigma = 5, 2
    table, R = ti_mod.bump_table(sigma)
    joints, counts = render_case(h, w, K, seed=h * w)
    got = render(pkg, joints, counts, table, R, K, h, w)
    want = np.zeros_like(got)
    ys, xs = np.mgrid[0:h, 0:w]
    for b in range(len(counts)):
        for x, y, vis, k in ((*joints[b, p, k], k) for p in range(counts[b]) for k in range(K)):
            if vis > 0 and 0 <= x < w and 0 <= y < h:
                dy, dx = ys - y + R, xs - x + R
                inside = (dy >= 0) & (dy < 2 * R + 1) & (dx >= 0) & (dx < 2 * R + 1)
                bump = np.where(inside, table[np.clip(dy, 0, 2 * R), np.clip(dx, 0, 2 * R)], np.float32(0))
                want[b, k] = np.maximum(want[b, k], bump)
    assert same_bits(got, want)


def test_staging_reuse_keeps_earlier_batches(pkg, ti_mod):  # noqa: F811
    """Three batch builds in a row without a synchronisation between them (the third reuses the first's staging buffer): each
    batch's outputs equal those of a fresh builder that built only that batch, i.e. the outputs do not depend on which staging
    buffer a batch went through or on what went through it before.  This does not prove the event ordering in `_staging`: by the
    third build the first copy has usually finished, and a test cannot force that race; the ordering rests on the code."""
    def batch(k):
        sizes = [(120 + 10 * k, 90 + 7 * i) for i in range(4)]
        samples = [pkg.synth.synth_train_sample(h, w, 2 + i, 100 * k + i, holes=1) for i, (h, w) in enumerate(sizes)]
        params = [ti_mod.AugParams(min(h, w) / 200 * (0.8 + 0.1 * i), 10.0 * (i - k), (w / 2 + k, h / 2 - i), bool((i + k) % 2)) for i, (h, w) in enumerate(sizes)]
        return samples, params

    ti = ti_mod.TrainInput(128, [1 / 4, 1 / 2], device=DEV)
    built = [ti.build(*batch(k)) for k in range(3)]
    torch.cuda.synchronize()
    for k in range(3):
        fresh = ti_mod.TrainInput(128, [1 / 4, 1 / 2], device=DEV).build(*batch(k))
        torch.cuda.synchronize()
        assert torch.equal(built[k][0], fresh[0]), k
        for i in range(2):
            assert torch.equal(built[k][1][i], fresh[1][i]) and torch.equal(built[k][2][i], fresh[2][i]), (k, i)
            assert torch.equal(built[k][3][i].packed, fresh[3][i].packed) and torch.equal(built[k][3][i].counts, fresh[3][i].counts)
    assert not torch.equal(built[0][0], built[1][0])


def test_training_step_on_a_device_built_batch(pkg, ti_mod, golden):  # noqa: F811
    """One KeypointsModule.training_step on the device-built batch returns exactly the metrics of the same step on the host-built
    batch (oracle warp + numpy generators + batch_to_device) from the same initial weights: the inputs are bit-identical."""
    meta, _ = golden
    km = importlib.import_module(PKG + ".keypoints.model")
    cases = [c for c in meta["cases"] if c["mode"] == "train"]
    ti, mode = golden_transform(ti_mod, meta, cases[0], device=DEV)
    samples = [golden_sample(pkg, meta, c) for c in cases]
    params = [golden_draw(mode, c)[0] for c in cases]
    K = meta["num_kpts"]

    host = [oracle_sample(ti, s, p) for s, p in zip(samples, params)]
    gens = [pkg.keypoints.targets.HeatmapGenerator(K, s, meta["sigma"]) for s in ti.hm_sizes]
    host_batch = (torch.from_numpy(np.stack([normalized(u8, ti.mean, ti.std) for u8, _, _ in host])),
                  [torch.from_numpy(np.stack([gens[i](ints[i]) for _, _, ints in host])) for i in range(2)],
                  [torch.from_numpy(np.stack([m[i] for _, m, _ in host])) for i in range(2)],
                  [[ints[i] for _, _, ints in host] for i in range(2)])

    def step(make_batch):
        net = pkg.HigherHRNet(K, 32)
        net.load_state_dict({k: torch.from_numpy(pkg.synth.synth_param(k, v.shape, 0)) for k, v in net.state_dict().items()})
        model = km.KeypointsModel(net)
        model.to_CUDA(0)
        model.net.train()
        module = km.KeypointsModule(model, pkg.AEKeypointsLoss(), torch.optim.Adam(model.net.parameters(), lr=1e-3))
        return module.training_step(make_batch(module), 0)

    on_host = step(lambda module: module.batch_to_device(host_batch))
    on_device = step(lambda module: ti.build(samples, params))
    assert set(on_device) == {"loss", "hm_0_loss", "hm_1_loss", "push_0_loss", "pull_0_loss"}
    assert on_device == on_host and all(np.isfinite(v) for v in on_device.values())
