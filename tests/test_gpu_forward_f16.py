"""-m gpu: the fp16 inference engine (HH_DTYPE_F16, HigherHRNet / ClassificationHRNet(dtype="fp16")) against the fp32 oracle under the
fp16 budgets of tests/forward_f16_budget.py, which the bf16 engine fails; the properties that need no reference; bf16 and fp16 handles
side by side; set_engine_dtype; the forward -> decode chain; the Python API; and overflow, which must show.

The engine / budget ratios the first two tests print are recorded in profiles/forward_f16.md."""
import contextlib
import hashlib
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import forward_budget as fb
import forward_f16_budget as f16
from conftest import PKG, REPO
from oracle import decode as orc
from oracle import forward as ofw

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@contextlib.contextmanager
def _env(env):
    os.environ.update(env)
    try:
        yield
    finally:
        for k in env:
            del os.environ[k]


def _net(pkg, kind, C, seed, dtype="fp16", env=None):
    """a fresh handle; the HH_* switches are read once, in its construction"""
    with _env(env or {}):
        net = pkg.ClassificationHRNet(C, 1000, dtype=dtype) if kind == "cls" else pkg.HigherHRNet(17, C, dtype=dtype)
        net.load_state_dict(fb.state_dict(C, seed, kind == "cls"))
        return net.to(DEV).eval()


_nets = {}


def _shared_net(pkg, kind, C, seed, dtype="fp16", env=()):
    key = (kind, C, seed, dtype, tuple(env))
    if key not in _nets:
        _nets[key] = _net(pkg, kind, C, seed, dtype, dict(env))
    return _nets[key]


def _run(net, kind, x):
    """-> the raw outputs, cloned: (init_heatmaps, deconv_heatmaps) or (logits,)"""
    with torch.no_grad():
        out = net.forward_raw(x) if kind == "pose" else (net(x),)
    return [t.clone() for t in out]


def _named(kind, out):
    if kind == "pose":
        return {"hm_q": out[0][:, :17].cpu().numpy(), "tags": out[0][:, 17:].cpu().numpy(), "hm_h": out[1].cpu().numpy()}
    return {"logits": out[0].cpu().numpy()}


def _same_bits(a, b, what):
    if torch.equal(a, b):
        return
    d = (a != b) | (a.isnan() != b.isnan())
    idx = d.nonzero()
    first = tuple(idx[0].tolist())
    raise AssertionError(f"{what}: {int(d.sum())} of {d.numel()} values differ, first at {first}: {a[first].item()!r} vs {b[first].item()!r}; "
                         f"NaNs {int(a.isnan().sum())} / {int(b.isnan().sum())}; differing index range {idx.min(0).values.tolist()} .. {idx.max(0).values.tolist()}")


# ---------------------------------------------------------------- 1, 2, 3: against the oracle
@pytest.mark.parametrize("case", f16.LATTICE_F16, ids=f16.case_id)
def test_outputs_vs_oracle_within_fp16_budget(pkg, case):
    """Every LATTICE_F16 shape on the default plan of a fresh fp16 handle built under HH_POISON_WS=1 (a value no kernel writes is a NaN,
    which check() counts as an infinite error) against the fp32 oracle, all five figures under budget_f16."""
    kind, C, B, H, W = case
    seed, iseed = f16.seeds(case)
    cls = kind == "cls"
    ref, _ = f16.tensors_f16((B, H, W), C, seed, iseed, cls)
    net = _net(pkg, kind, C, seed, "fp16", {"HH_POISON_WS": "1"})
    got = _named(kind, _run(net, kind, fb.images((B, H, W), iseed).to(DEV)))
    ratios = {}
    for name in f16.OUTPUTS[kind]:
        r = fb.check(got[name], ref[name], f16.budget_f16(name, (B, H, W), C, seed, iseed, cls), f"fp16 {f16.case_id(case)} {name}")
        ratios[name] = {k: round(v, 2) for k, v in r.items()}
    print(f"fp16 engine / budget {f16.case_id(case)}: {ratios}")


TAP_SHAPES = [(1, 64, 64), (4, 32, 32)]


@pytest.mark.parametrize("shape", TAP_SHAPES, ids=lambda s: "{}x{}x{}".format(*s))
def test_taps_vs_oracle_within_per_tap_fp16_budget(pkg, shape):
    """Every tap of the fp16 engine against the oracle's tensor of that name, each under its own budget_f16: one kernel left multiplying
    fp16 bits as bf16 (or reading a tap as bf16) shows at its first tap."""
    seed, iseed = 1 + TAP_SHAPES.index(shape) % 3, 80 + TAP_SHAPES.index(shape)
    ref, _ = f16.tensors_f16(shape, 32, seed, iseed)
    net = _net(pkg, "pose", 32, seed, "fp16", {"HH_POISON_WS": "1"})
    net.set_taps(True)
    _run(net, "pose", fb.images(shape, iseed).to(DEV))
    torch.cuda.synchronize()
    taps = net.read_taps()
    names = [n for n in taps if n in ref and n != "deconv#1"]
    assert len(names) >= 60, sorted(taps)
    worst = {}
    for name in names:
        r = fb.check(taps[name], ref[name], f16.budget_f16(name, shape, 32, seed, iseed), f"fp16 {shape} tap {name}")
        group = name.split(".blocks")[0].split("#")[0]
        for k, v in r.items():
            worst[group, k] = max(worst.get((group, k), 0.0), v)
    groups = sorted({g for g, _ in worst})
    print(f"fp16 engine / budget, taps at {shape}: " + "; ".join(f"{g} " + " ".join(f"{k} {worst[g, k]:.2f}" for k in fb.FIGURES) for g in groups))


def test_bf16_engine_fails_the_fp16_budget(pkg):
    """The test has teeth on the device: the bf16 engine's outputs at 3x64x64 are over budget_f16."""
    case = f16.LATTICE_F16[0]
    kind, C, B, H, W = case
    seed, iseed = f16.seeds(case)
    ref, _ = f16.tensors_f16((B, H, W), C, seed, iseed)
    got = _named(kind, _run(_shared_net(pkg, kind, C, seed, "bf16"), kind, fb.images((B, H, W), iseed).to(DEV)))
    for name in f16.OUTPUTS[kind]:
        fb.check(got[name], ref[name], fb.budget(name, (B, H, W), C, seed, iseed), f"bf16 {name}")  # (it is a sound bf16 engine)
        with pytest.raises(AssertionError):
            fb.check(got[name], ref[name], f16.budget_f16(name, (B, H, W), C, seed, iseed), f"bf16 engine under the fp16 budget, {name}")


# ---------------------------------------------------------------- 4: properties that need no reference
def test_images_of_a_batch_are_independent(pkg):
    B, H, W = 5, 32, 256
    net = _shared_net(pkg, "pose", 32, 1)
    x = fb.images((B, H, W), 61).to(DEV)
    batch = _run(net, "pose", x)
    again = _run(net, "pose", x)
    for t, (u, v) in enumerate(zip(batch, again)):
        assert not u.isnan().any()
        _same_bits(u, v, f"output {t}: second call vs first")
    for b in range(B):
        one = _run(net, "pose", x[b:b + 1].contiguous())
        for t, (u, v) in enumerate(zip(batch, one)):
            _same_bits(u[b:b + 1], v, f"output {t}: slot {b} of the batch vs that image alone")


def test_multi_lane_equals_single_lane(pkg):
    lib = pkg._lib.load()
    net = _net(pkg, "pose", 32, 1)
    x = fb.images((2, 128, 128), 68).to(DEV)
    multi = _run(net, "pose", x)
    pkg._lib.check(lib.hh_set_multi_lane(net._h, 0))
    single = _run(net, "pose", x)
    for t, (u, v) in enumerate(zip(multi, single)):
        _same_bits(u, v, f"output {t}: multi-lane vs hh_set_multi_lane(0)")


@pytest.mark.parametrize("shape", [(5, 32, 256), (3, 64, 64)], ids=lambda s: "{}x{}x{}".format(*s))
def test_tall_layout_vs_per_image_layout(pkg, shape):
    x = fb.images(shape, 90).to(DEV)
    ref = _run(_shared_net(pkg, "pose", 32, 1), "pose", x)
    got = _run(_shared_net(pkg, "pose", 32, 1, "fp16", (("HH_NO_BB_TALL", "1"),)), "pose", x)
    for t, (u, v) in enumerate(zip(got, ref)):
        _same_bits(u, v, f"{shape} output {t}: HH_NO_BB_TALL=1 vs the default layout")


def test_unfused_plans_within_budget(pkg):
    """The plan without the head fold, the final-layer fusion, the fused up-sum, the junction pairs, the fused 64-channel block, the
    two-buffer convs and the merged fusion convs -- the generic conv / upadd kernels in their fp16 form -- under the same budget."""
    case = f16.LATTICE_F16[0]
    kind, C, B, H, W = case
    seed, iseed = f16.seeds(case)
    ref, _ = f16.tensors_f16((B, H, W), C, seed, iseed)
    env = {k: "1" for k in ("HH_NO_HEAD_FOLD", "HH_NO_FINAL_FUSE", "HH_NO_FUSED_UPSUM", "HH_NO_JUNC_PAIR", "HH_NO_BB64", "HH_NO_CONV_DB", "HH_NO_FUSION_MERGE")}
    got = _named(kind, _run(_net(pkg, kind, C, seed, "fp16", env), kind, fb.images((B, H, W), iseed).to(DEV)))
    for name in f16.OUTPUTS[kind]:
        fb.check(got[name], ref[name], f16.budget_f16(name, (B, H, W), C, seed, iseed), f"fp16 unfused plan {name}")


# ---------------------------------------------------------------- 5, 6: handles
def _digest(tensors) -> str:
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.cpu().numpy().tobytes())
    return h.hexdigest()


_CHILD = """
import hashlib, importlib, sys
sys.path.insert(0, {repo!r}); sys.path.insert(0, {tests!r})
import torch
import forward_budget as fb
pkg = importlib.import_module({pkg!r})
net = pkg.HigherHRNet(17, 32)
net.load_state_dict(fb.state_dict(32, 1))
net = net.to("cuda:0").eval()
with torch.no_grad():
    out = net.forward_raw(fb.images((2, 128, 128), 68).to("cuda:0"))
h = hashlib.sha256()
for t in out:
    h.update(t.cpu().numpy().tobytes())
print("digest", h.hexdigest())
"""


def test_bf16_and_fp16_handles_side_by_side(pkg):
    """A bf16 and an fp16 net alive together, called alternately: each repeats its own bits, and the bf16 net's are those of a process
    that never created an fp16 handle (a fresh child process)."""
    x = fb.images((2, 128, 128), 68).to(DEV)
    nb, nf = _net(pkg, "pose", 32, 1, "bf16"), _net(pkg, "pose", 32, 1, "fp16")
    first = None
    for _ in range(3):
        cur = (_run(nb, "pose", x), _run(nf, "pose", x))
        if first is None:
            first = cur
        for which, (a, b) in enumerate(zip(cur, first)):
            for t, (u, v) in enumerate(zip(a, b)):
                _same_bits(u, v, f"{('bf16', 'fp16')[which]} net output {t}: a later alternation vs the first")
    assert not torch.equal(first[0][0], first[1][0])  # (two formats, two results)
    child = subprocess.run([sys.executable, "-c", _CHILD.format(repo=REPO, tests=os.path.join(REPO, "tests"), pkg=PKG)],
                           capture_output=True, text=True, timeout=300)
    assert child.returncode == 0, child.stderr[-2000:]
    digest = [line.split()[1] for line in child.stdout.splitlines() if line.startswith("digest ")]
    assert digest == [_digest(first[0])], (digest, _digest(first[0]))


def test_set_engine_dtype_gives_the_bits_of_fresh_handles(pkg):
    x = fb.images((2, 128, 128), 68).to(DEV)
    fresh = {d: _run(_net(pkg, "pose", 32, 1, d), "pose", x) for d in ("bf16", "fp16")}
    net = _net(pkg, "pose", 32, 1, "bf16")
    for d in ("bf16", "fp16", "bf16"):
        net.set_engine_dtype(d)
        assert net.engine_dtype == d
        for t, (u, v) in enumerate(zip(_run(net, "pose", x), fresh[d])):
            _same_bits(u, v, f"after set_engine_dtype({d!r}), output {t}: vs a fresh {d} net")


# ---------------------------------------------------------------- 7: forward -> decode
FP8_MIN_COVER = 0.8  # the project's own bound for the fp8 chain (test_gpu_parity.py); fp16 must meet it a fortiori


def test_chained_forward_decode_on_person_like_maps(pkg):
    """fp16 forward -> hh_decode on the pass-through net (constructed people carried from the images to the maps): the device decode
    equals the oracle's decode of the same maps bit for bit, and every person the fp32 maps decode to has an fp16 counterpart holding
    at least FP8_MIN_COVER of its detected joints within 2 px."""
    B, hq, wq = 4, 64, 64
    nets = {d: pkg.HigherHRNet(17, 32, dtype=d) for d in ("bf16", "fp16")}
    sd = {k: torch.from_numpy(v) for k, v in
          pkg.synth.synth_passthrough_state_dict({k: tuple(v.shape) for k, v in nets["fp16"].state_dict().items()}, 17, 0).items()}
    imgs = pkg.synth.synth_passthrough_images(B, hq, wq, [3, 2, 1, 3], 17, 1)[0]
    with torch.no_grad():
        (r_hq, r_hh), r_tags = ofw.higher_hrnet(torch.from_numpy(imgs), sd, 17)
    parser = pkg.MPPEHeatmapParser(17, 30, 0.05, 0.5)
    counts = {}
    worst_cover = 1.0
    for d, net in nets.items():
        net.load_state_dict(sd)
        net = net.to(DEV).eval()
        (g_hq, g_hh), g_tags = net(torch.from_numpy(imgs).to(DEV))
        got = parser.to_lists(*parser.decode_batch_device(g_hq, g_hh, [g_tags]))
        for b in range(B):
            oj, os_ = orc.decode(g_hq[b].cpu().numpy(), g_hh[b].cpu().numpy(), [g_tags[b].cpu().numpy()], max_people=30, det_thr=0.05, tag_thr=0.5)
            assert np.array_equal(got[b][0], oj) and np.array_equal(got[b][1], os_), (d, b)
            rj, _ = orc.decode(r_hq[b].numpy(), r_hh[b].numpy(), [r_tags[b].numpy()], max_people=30, det_thr=0.05, tag_thr=0.5)
            counts.setdefault(b, [rj.shape[0]]).append(oj.shape[0])
            if d != "fp16":
                continue
            for pr in rj:
                det = pr[:, 2] > 0
                if not det.any():
                    continue
                best = 0.0
                for po in oj:
                    near = det & (po[:, 2] > 0) & (np.abs(po[:, 0] - pr[:, 0]) <= 2.0) & (np.abs(po[:, 1] - pr[:, 1]) <= 2.0)
                    best = max(best, near.sum() / det.sum())
                worst_cover = min(worst_cover, best)
    print("fp16 chained: groups (fp32 oracle, bf16 engine, fp16 engine) per image:", [tuple(counts[b]) for b in range(B)],
          " least share of a reference person's joints found in one fp16 person:", round(worst_cover, 3))
    assert worst_cover >= FP8_MIN_COVER, worst_cover


# ---------------------------------------------------------------- 8: API
def test_inference_model_on_an_fp16_net(pkg):
    net = _net(pkg, "pose", 32, 1)
    model = pkg.InferenceKeypointsModel(net, det_thr=0.05, tag_thr=0.5, use_flip=False, input_size=128, device=DEV)
    rs = np.random.RandomState(7)
    images = [rs.randint(0, 255, s + (3,)).astype(np.uint8) for s in ((96, 128), (128, 96), (96, 128))]
    batched = model.infer_images(images, max_batch=3)
    assert len(batched) == len(images) and net.engine_dtype == "fp16"
    for im, rb in zip(images, batched):
        r1 = model(im, None)
        for f in ("kpts_coords", "kpts_scores", "kpts_tags", "obj_scores"):
            a, b = getattr(rb, f), getattr(r1, f)
            assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), f
        assert torch.equal(rb.model_input_image, r1.model_input_image)


@pytest.mark.parametrize("case", [c for c in f16.LATTICE_F16 if c[0] == "cls"], ids=f16.case_id)
def test_fp16_classifier_has_the_oracle_top1(pkg, case):
    kind, C, B, H, W = case
    seed, iseed = f16.seeds(case)
    ref, _ = f16.tensors_f16((B, H, W), C, seed, iseed, True)
    logits = _run(_shared_net(pkg, "cls", C, seed), "cls", fb.images((B, H, W), iseed).to(DEV))[0].cpu().numpy()
    assert np.array_equal(logits.argmax(1), ref["logits"].argmax(1))


def test_modules_eval_dtype(pkg):
    """KeypointsModule(eval_dtype="fp16"): validation_step infers on the fp16 engine; eval_dtype=None is the module without the argument,
    bit for bit.  ClassificationModule takes the same argument."""
    kp = importlib.import_module(PKG + ".keypoints")
    B, S = 2, 128
    imgs = fb.images((B, S, S), 5)
    hms, masks, joints = pkg.synth.synth_train_targets(B, 17, S, 3, seed=2)
    batch = (imgs.to(DEV), [torch.from_numpy(h).to(DEV) for h in hms], [torch.from_numpy(m).to(DEV) for m in masks], joints)

    def step(**kw):
        net = _net(pkg, "pose", 32, 1, "bf16")
        module = kp.KeypointsModule(kp.KeypointsModel(net), pkg.AEKeypointsLoss(), torch.optim.SGD(net.parameters(), lr=0.0), **kw)
        metrics, results = module.validation_step(batch)
        return net, metrics, results

    net, metrics, results = step(eval_dtype="fp16")
    assert net.engine_dtype == "fp16" and len(results) == B
    assert set(metrics) == {"loss", "hm_0_loss", "hm_1_loss", "push_0_loss", "pull_0_loss"} and all(np.isfinite(v) for v in metrics.values())
    for t, (u, v) in enumerate(zip(_run(net, "pose", batch[0]), _run(_shared_net(pkg, "pose", 32, 1), "pose", batch[0]))):
        _same_bits(u, v, f"the module's net after eval_dtype='fp16', output {t}: vs an fp16 net")
    net_none, m_none, _ = step(eval_dtype=None)
    net_plain, m_plain, _ = step()
    assert net_none.engine_dtype == net_plain.engine_dtype == "bf16" and m_none == m_plain
    assert m_none != metrics  # (bf16 and fp16 maps differ)
    cls = importlib.import_module(PKG + ".classification")
    cnet = _net(pkg, "cls", 32, 1, "bf16")
    cls.ClassificationModule(cls.ClassificationModel(cnet), cls.ClassificationLoss(), torch.optim.SGD(cnet.parameters(), lr=0.0), eval_dtype="fp16")
    assert cnet.engine_dtype == "fp16"


# ---------------------------------------------------------------- 9: overflow
def test_overflow_is_visible(pkg):
    """Images scaled by the smallest power of two at which the fp16 emulation's outputs are non-finite (computed here, on the CPU): the
    engine's outputs are non-finite too -- never a finite, plausible map from an overflowed activation."""
    shape = (1, 32, 32)
    sd, x = fb.state_dict(32, 1), fb.images(shape, 3)
    scale = None
    for k in range(0, 40):
        emu = f16.forward_f16(x * 2.0**k, sd)
        if not all(np.isfinite(emu[n]).all() for n in ("hm_q", "hm_h", "tags")):
            scale = 2.0**k
            break
    assert scale is not None and scale > 1, "the emulation never overflowed"
    net = _shared_net(pkg, "pose", 32, 1)
    fine = _run(net, "pose", x.to(DEV))
    assert all(torch.isfinite(t).all() for t in fine)
    out = _run(net, "pose", (x * scale).to(DEV))
    print(f"fp16 overflow: images x {scale:g}; non-finite engine values: {[int((~torch.isfinite(t)).sum()) for t in out]} of {[t.numel() for t in out]}")
    assert not all(torch.isfinite(t).all() for t in out), f"images x {scale:g}: the emulation overflows, the engine's outputs are all finite"


def test_finalize_refuses_a_weight_beyond_the_fp16_range(pkg):
    name = "backbone.stages.1.blocks.0.scales_blocks.1.2.conv1"
    bn = name.replace("conv1", "bn1")
    sd = fb.state_dict(32, 1)
    sd = {k: v.clone() for k, v in sd.items()}
    sd[bn + ".weight"][3], sd[bn + ".running_var"][3], sd[name + ".weight"][3, 5, 1, 1] = 1.0, 1.0, 1e5  # folded: 1e5 / sqrt(1 + 1e-5)
    x = fb.images((1, 32, 32), 3).to(DEV)
    net = pkg.HigherHRNet(17, 32, dtype="fp16")
    net.load_state_dict(sd)
    net = net.to(DEV).eval()
    with pytest.raises(pkg._lib.HHError, match=name.replace(".", r"\.") + r"\.weight.*fp16 range"):
        net(x)
    # a summed stride-2 conv of a fusion layer (packed as one conv over concatenated inputs): the message names ITS parameter
    sd2 = fb.state_dict(32, 1)
    sd2 = {k: v.clone() for k, v in sd2.items()}
    fname = "backbone.stages.2.blocks.1.scales_fusion_layers.2.0.1"
    assert sd2[fname + ".0.weight"].shape == (128, 32, 3, 3)
    sd2[fname + ".1.weight"][7], sd2[fname + ".1.running_var"][7], sd2[fname + ".0.weight"][7, 2, 0, 2] = 1.0, 1.0, -1e5
    net.load_state_dict(sd2)
    with pytest.raises(pkg._lib.HHError, match=fname.replace(".", r"\.") + r"\.0\.weight.*fp16 range"):
        net(x)
    with pytest.raises(pkg._lib.HHError, match="not an fp8 handle"):
        _shared_net(pkg, "pose", 32, 1).calibrate(x)
    bf = pkg.HigherHRNet(17, 32)  # bf16 has the range
    bf.load_state_dict(sd)
    assert all(torch.isfinite(t).all() for t in _run(bf.to(DEV).eval(), "pose", x))
