"""The mosaic of the training input composed on the device (hh_mosaic_u8_batch, keypoints/train_input.py: Mosaic, mosaic_probability):
the canvases bit-identical to tests/cv_resize.py over a lattice of tile sizes, the built batch bit-identical to
cv_resize.mosaic_reference -> oracle.transforms.warp_affine -> the numpy generators and to the reference-run golden.  Everything here
is an equality of bits: resize and warps are integer arithmetic."""
import importlib
import random

import numpy as np
import pytest
import torch

import cv_resize as cv
from conftest import PKG
from test_gpu_train_input import normalized, oracle_sample, same_bits
from train_input_helpers import ti_mod  # noqa: F401
from train_mosaic_helpers import golden_pool, mosaic_golden  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 0x5B  # neither 0 nor 255: an unwritten mask byte shows as well

SIZES_64 = [(64, 64), (128, 128), (128, 100), (100, 128), (40, 56), (150, 97), (300, 260), (256, 256), (63, 65), (65, 63), (129, 127), (1, 1), (1, 200),
            (200, 1), (2, 2)]


def tile(h, w, kind, seed):
    """A noise image with a crowd mask of one of four kinds: all true, all false, a rectangular hole, single-pixel holes (and, in
    the hole, single true pixels)."""
    rs = np.random.RandomState(7000 + seed)
    img = rs.randint(0, 256, (h, w, 3)).astype(np.uint8)
    mask = np.ones((h, w), bool)
    if kind == 1:
        mask[:] = False
    elif kind == 2:
        mask[h // 4:h // 4 + max(h // 2, 1), w // 3:w // 3 + max(w // 2, 1)] = False
        mask[rs.randint(0, h, 3), rs.randint(0, w, 3)] = True
    elif kind == 3:
        mask[rs.randint(0, h, 5), rs.randint(0, w, 5)] = False
    return img, mask, np.zeros((0, 17, 3))


def compose(pkg, ti_mod, mosaics, S):  # noqa: F811
    """hh_mosaic_u8_batch through the C-ABI, all mosaics in ONE launch, into canvases prefilled with SENTINEL
    -> [(canvas uint8 [2S,2S,3], mask canvas uint8 [2S,2S])]."""
    lib = pkg._lib.load()
    n = len(mosaics)
    flat = [t for m in mosaics for t in m]
    sizes = [t[0].size for t in flat] + [t[1].size for t in flat]
    offs = np.cumsum([0] + sizes)
    desc_off = (int(offs[-1]) + 63) // 64 * 64
    canvas_off = (desc_off + 112 * n + 63) // 64 * 64
    total = canvas_off + n * 16 * S * S
    host = np.full(total, SENTINEL, np.uint8)
    descs = host[desc_off:desc_off + 112 * n].view(ti_mod._MOSAIC_DESC)
    for i, (img, mask, _) in enumerate(flat):
        host[offs[i]:offs[i + 1]] = img.reshape(-1)
        host[offs[len(flat) + i]:offs[len(flat) + i + 1]] = (mask * 255).astype(np.uint8).reshape(-1)
    for m in range(n):
        tiles = [(int(offs[4 * m + t]), int(offs[len(flat) + 4 * m + t]), *flat[4 * m + t][0].shape[:2]) for t in range(4)]
        descs[m] = (tiles, canvas_off + m * 16 * S * S, canvas_off + m * 16 * S * S + 12 * S * S)
    raw = torch.from_numpy(host).to(DEV)
    pkg._lib.check(lib.hh_mosaic_u8_batch(raw.data_ptr(), raw.data_ptr() + desc_off, descs.ctypes.data, n, S, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    back = raw.cpu().numpy()
    assert np.array_equal(back[:canvas_off], host[:canvas_off])  # nothing but the canvases is written
    out = []
    for m in range(n):
        at = canvas_off + m * 16 * S * S
        out.append((back[at:at + 12 * S * S].reshape(2 * S, 2 * S, 3), back[at + 12 * S * S:at + 16 * S * S].reshape(2 * S, 2 * S)))
    return out


def check_compose(pkg, ti_mod, sizes, S):  # noqa: F811
    """`sizes` twice over, four to a mosaic: with len(sizes) % 4 == 3 every size sits in two different quadrants, with two
    different mask kinds."""
    assert len(sizes) % 4 == 3
    seq = list(sizes) * 2 + list(sizes[:2])
    tiles = [tile(h, w, i % 4, 100 * S + i) for i, (h, w) in enumerate(seq)]
    mosaics = [tiles[i:i + 4] for i in range(0, len(tiles), 4)]
    assert len(mosaics) > 1
    got = compose(pkg, ti_mod, mosaics, S)
    for m, (canvas, canvas_mask) in enumerate(got):
        want, want_mask, _ = cv.mosaic_reference(mosaics[m], S)
        where = (S, m, [t[0].shape[:2] for t in mosaics[m]])
        assert same_bits(canvas, want), where
        assert same_bits(canvas_mask, want_mask.astype(np.uint8) * 255), where
    return got


def test_compose_kernel_lattice_s64(pkg, ti_mod):  # noqa: F811
    got = check_compose(pkg, ti_mod, SIZES_64, 64)
    masks = np.stack([m for _, m in got])
    assert set(np.unique(masks)) == {0, 255}


@pytest.mark.parametrize("S", [96, 128])
def test_compose_kernel_other_sizes(pkg, ti_mod, S):  # noqa: F811
    check_compose(pkg, ti_mod, [(S, S), (2 * S, 2 * S), (2 * S, 100), (150, 97), (300, 260), (1, 200), (129, 127)], S)


def test_compose_kernel_s512(pkg, ti_mod):  # noqa: F811
    sources = [(480, 640), (1024, 1024), (427, 640), (640, 360)]
    mosaic = [tile(h, w, (2, 3, 0, 2)[i], 900 + i) for i, (h, w) in enumerate(sources)]
    (canvas, canvas_mask), = compose(pkg, ti_mod, [mosaic], 512)
    want, want_mask, _ = cv.mosaic_reference(mosaic, 512)
    assert same_bits(canvas, want) and same_bits(canvas_mask, want_mask.astype(np.uint8) * 255)


# ------------------------------------------------------------------ build()
def host_entry(ti_mod, ti, entry, p):  # noqa: F811
    """One batch entry on the host: a Mosaic through cv_resize.mosaic_reference, then the oracle warp of test_gpu_train_input
    -> (uint8 image [S,S,3], [mask fp32 [s,s]], [int joints])."""
    sample = cv.mosaic_reference(entry.tiles, ti.out_size) if isinstance(entry, ti_mod.Mosaic) else entry
    return oracle_sample(ti, sample, p)


def check_batch(pkg, ti_mod, ti, entries, params, built):  # noqa: F811
    """Images, every stage's masks and heatmaps, and the packed joints of a built batch against the host."""
    loss = importlib.import_module(PKG + ".keypoints.loss")
    images, heatmaps, masks, joints = built
    host = [host_entry(ti_mod, ti, e, p) for e, p in zip(entries, params)]
    images = images.cpu().numpy()
    for b, (u8, _, _) in enumerate(host):
        assert same_bits(images[b], normalized(u8, ti.mean, ti.std)), b
    for i, s in enumerate(ti.hm_sizes):
        gen = pkg.keypoints.targets.HeatmapGenerator(ti.num_kpts, s, ti.sigmas[i])
        got_masks, got_hms = masks[i].cpu().numpy(), heatmaps[i].cpu().numpy()
        for b, (_, ref_masks, ints) in enumerate(host):
            assert same_bits(got_masks[b], ref_masks[i]), (b, i)
            assert same_bits(got_hms[b], gen(ints[i])), (b, i)
        packed, counts = loss.pack_joints([ints[i] for _, _, ints in host], ti.num_kpts, s, s)
        assert same_bits(joints[i].packed.cpu().numpy(), packed) and same_bits(joints[i].counts.cpu().numpy(), counts)


def raw_samples(pkg, count, seed, integer=()):
    sizes = [(120, 90), (256, 256), (97, 150), (128, 128), (60, 200), (300, 260), (128, 100), (33, 47)]
    out = []
    for i in range(count):
        h, w = sizes[(i + seed) % len(sizes)]
        img, mask, joints = pkg.synth.synth_train_sample(h, w, (3, 0, 5, 1)[i % 4], 500 + 10 * seed + i, holes=(2, -1, 0, 1)[(i + seed) % 4])
        out.append((img, mask, joints.astype(np.int64) if i in integer else joints))
    return out


def lattice_params(ti_mod, S, shapes):  # noqa: F811
    """Rotation +-30 degrees, scale 0.75 / 1.5, both flips, the centre off the middle."""
    out = []
    for b, (h, w) in enumerate(shapes):
        scale = min(h, w) / 200 * (0.75, 1.5)[(b // 2) % 2]
        out.append(ti_mod.AugParams(scale, (-30.0, 30.0)[(b % 2) ^ (b // 2 % 2)], (w / 2 + 3 - 2 * b, h / 2 - 5 + 3 * b), bool((b + b // 2) % 2)))
    return out


def test_build_with_mosaics_against_the_host(pkg, ti_mod):  # noqa: F811
    S = 128
    ti = ti_mod.TrainInput(S, [1 / 4, 1 / 2], device=DEV)
    r = raw_samples(pkg, 10, 0, integer=(3, 4))
    entries = [r[0], ti_mod.Mosaic(r[1:5]), r[5], ti_mod.Mosaic([r[6], r[7], r[6], r[9]])]  # (256,256) = 2S x 2S among the tiles; a repeat
    params = lattice_params(ti_mod, S, [r[0][0].shape[:2], (2 * S, 2 * S), r[5][0].shape[:2], (2 * S, 2 * S)])
    assert [(p.rot, p.scale, p.flip) for p in params[1::2]] == [(30.0, 256 / 200 * 0.75, True), (-30.0, 256 / 200 * 1.5, False)]
    built = ti.build(entries, params)
    torch.cuda.synchronize()
    assert ti.last_launches == 2 + 2 + 1
    check_batch(pkg, ti_mod, ti, entries, params, built)
    assert 0 < built[2][1][1].mean() < 1 and built[1][1][1].max() == 1.0  # the mosaic's mask is mixed and its heatmaps hold people
    # the raw samples are what they are in a batch without any mosaic
    plain = ti.build([entries[0], entries[2]], [params[0], params[2]])
    torch.cuda.synchronize()
    assert ti.last_launches == 2 + 2
    assert torch.equal(built[0][[0, 2]], plain[0])
    for i in range(2):
        assert torch.equal(built[1][i][[0, 2]], plain[1][i]) and torch.equal(built[2][i][[0, 2]], plain[2][i])


def golden_batch(pkg, ti_mod, meta, **kw):  # noqa: F811
    ti = ti_mod.TrainInput(meta["out_size"], meta["hm_resolutions"], num_kpts=meta["num_kpts"], sigma=meta["sigma"], **meta["transform"],
                           mosaic_probability=meta["mosaic_probability"], **kw)
    entries, params = [], []
    for case in meta["cases"]:
        pool = golden_pool(pkg, meta, case)
        np.random.seed(case["rng_seed"])
        random.seed(case["rng_seed"])
        e, p = ti.train.choose([pool[case["item"]]], pool)
        entries += e
        params += p
    return ti, entries, params


def test_golden_cases_bit_identical(pkg, ti_mod, mosaic_golden):  # noqa: F811
    meta, data = mosaic_golden
    loss = importlib.import_module(PKG + ".keypoints.loss")
    ti, entries, params = golden_batch(pkg, ti_mod, meta, device=DEV)
    assert all(isinstance(e, ti_mod.Mosaic) for e in entries)
    images, heatmaps, masks, joints = ti.build(entries, params)
    torch.cuda.synchronize()
    for b, case in enumerate(meta["cases"]):
        tag = case["tag"]
        assert same_bits(images[b].cpu().numpy(), normalized(data[f"{tag}.image_u8"], ti.mean, ti.std)), tag
        for i in range(len(ti.hm_sizes)):
            assert same_bits(masks[i][b].cpu().numpy(), data[f"{tag}.mask{i}"].astype(np.float32)), (tag, i)
            assert same_bits(heatmaps[i][b].cpu().numpy(), data[f"{tag}.hm{i}"]), (tag, i)
    for i, s in enumerate(ti.hm_sizes):
        packed, counts = loss.pack_joints([data[f"{c['tag']}.joints_i{i}"] for c in meta["cases"]], meta["num_kpts"], s, s)
        assert same_bits(joints[i].packed.cpu().numpy(), packed) and same_bits(joints[i].counts.cpu().numpy(), counts)


def test_consecutive_builds(pkg, ti_mod):  # noqa: F811
    """A large mosaic batch, a smaller plain one, a mosaic one again, without a synchronisation in between: each is correct, and the
    first batch's tensors are what they were after the later builds."""
    S = 128
    ti = ti_mod.TrainInput(S, [1 / 4, 1 / 2], device=DEV)
    a, b, c = raw_samples(pkg, 14, 1), raw_samples(pkg, 2, 2), raw_samples(pkg, 5, 3)
    batches = [([ti_mod.Mosaic(a[0:4]), a[4], ti_mod.Mosaic(a[5:9]), ti_mod.Mosaic(a[9:13]), a[13]], None), (b, None), ([c[0], ti_mod.Mosaic(c[1:5])], None)]
    batches = [(e, lattice_params(ti_mod, S, [(2 * S, 2 * S) if isinstance(x, ti_mod.Mosaic) else x[0].shape[:2] for x in e])) for e, _ in batches]
    built = [ti.build(e, p) for e, p in batches]
    first = [t.clone() for t in (built[0][0], *built[0][1], *built[0][2])]
    torch.cuda.synchronize()
    for (e, p), out in zip(batches, built):
        check_batch(pkg, ti_mod, ti, e, p, out)
    again = [ti.build(e, p) for e, p in batches[1:]]
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(first, (built[0][0], *built[0][1], *built[0][2])))
    check_batch(pkg, ti_mod, ti, *batches[0], built[0])
    for (e, p), out in zip(batches[1:], again):
        check_batch(pkg, ti_mod, ti, e, p, out)


def test_train_mode_with_a_pool(pkg, ti_mod):  # noqa: F811
    S, seed = 128, 12345
    samples, pool = raw_samples(pkg, 8, 4), raw_samples(pkg, 6, 5, integer=(1, 2))
    ti = ti_mod.TrainInput(S, [1 / 4, 1 / 2], device=DEV, mosaic_probability=0.5)

    def seeded(fn):
        np.random.seed(seed)
        random.seed(seed)
        return fn()

    entries, params = seeded(lambda: ti.train.choose(samples, pool))
    kinds = [isinstance(e, ti_mod.Mosaic) for e in entries]
    assert any(kinds) and not all(kinds)
    got = seeded(lambda: ti.train(samples, pool))
    assert ti.last_launches == 2 + 2 + 1
    bytes_with = ti.last_h2d_bytes
    want = ti.build(entries, params)
    torch.cuda.synchronize()
    assert torch.equal(got[0], want[0])
    for i in range(2):
        assert torch.equal(got[1][i], want[1][i]) and torch.equal(got[2][i], want[2][i])
        assert torch.equal(got[3][i].packed, want[3][i].packed) and torch.equal(got[3][i].counts, want[3][i].counts)
    check_batch(pkg, ti_mod, ti, entries, params, got)

    # probability 0: the draws, the outputs, the launches and the copied bytes of the path without the parameter
    ti0 = ti_mod.TrainInput(S, [1 / 4, 1 / 2], device=DEV, mosaic_probability=0.0)
    plain = ti_mod.TrainInput(S, [1 / 4, 1 / 2], device=DEV)
    got0 = seeded(lambda: ti0.train(samples))
    launches0, bytes0 = ti0.last_launches, ti0.last_h2d_bytes
    want0 = seeded(lambda: plain.build(samples, [plain.train.draw(*s[0].shape[:2]) for s in samples]))
    torch.cuda.synchronize()
    assert launches0 == plain.last_launches == 2 + 2 and bytes0 == plain.last_h2d_bytes < bytes_with
    pixels = sum(s[0].size + s[1].size for s in samples)
    stage_joint_bytes = sum(j.packed.numel() * 4 + j.counts.numel() * 4 for j in want0[3])
    assert bytes0 == (pixels + 63) // 64 * 64 + 272 * len(samples) + stage_joint_bytes
    assert torch.equal(got0[0], want0[0])
    for i in range(2):
        assert torch.equal(got0[1][i], want0[1][i]) and torch.equal(got0[2][i], want0[2][i])
        assert torch.equal(got0[3][i].packed, want0[3][i].packed)


def test_training_step_on_a_device_built_mosaic_batch(pkg, ti_mod):  # noqa: F811
    """One KeypointsModule.training_step on the device-built batch (one mosaic, one raw) returns exactly the metrics of the same step on
    the batch built on the host from cv_resize.mosaic_reference: the inputs are bit-identical."""
    km = importlib.import_module(PKG + ".keypoints.model")
    S, K = 128, 17
    ti = ti_mod.TrainInput(S, [1 / 4, 1 / 2], device=DEV)
    r = raw_samples(pkg, 5, 6)
    entries = [ti_mod.Mosaic(r[0:4]), r[4]]
    params = lattice_params(ti_mod, S, [(2 * S, 2 * S), r[4][0].shape[:2]])
    host = [host_entry(ti_mod, ti, e, p) for e, p in zip(entries, params)]
    gens = [pkg.keypoints.targets.HeatmapGenerator(K, s, 2) for s in ti.hm_sizes]
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
    on_device = step(lambda module: ti.build(entries, params))
    assert set(on_device) == {"loss", "hm_0_loss", "hm_1_loss", "push_0_loss", "pull_0_loss"}
    assert on_device == on_host and all(np.isfinite(v) for v in on_device.values())
