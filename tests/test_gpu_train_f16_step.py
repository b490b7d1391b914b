"""-m gpu: the whole training step at the reference's precision -- fp16 activations (HigherHRNet.set_train_precision("fp16")) and the
reference's GradScaler sequence (KeypointsModule(precision="fp16")).

1. B = 2 at 128 x 128, W32, synth_param(., 5), synth_images(2, 128, 128, seed=1): the setup of tests/golden/train_step.npz (the reference in
   fp32) and train_step_autocast.npz (the reference under torch.autocast(float16)).  The fixed caps are the bf16 step's
   (test_train_step_matches_reference_autograd); the number that shows the feature is the rms deviation of the sampled outputs from the
   fp32 golden over the reference autocast step's own deviation: 7.1-7.4 for bf16 (three significand bits), about 1 for equal formats,
   asserted < 2.0 (one bit).  Not measured yet: no GPU run was possible while this file was written.
2. KeypointsModule(precision="fp16") with Adam and the AE loss on a synthetic batch: three steps, a skipped step at an oversized scale, the
   scaler state round trip, and precision="bf16" unchanged.
"""
import importlib
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, PKG
from oracle import forward as ofw

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
K = 17


def _net(pkg, seed, precision):
    net = pkg.HigherHRNet(K, 32)
    sd = {k: torch.from_numpy(pkg.synth.synth_param(k, v.shape, seed)) for k, v in net.state_dict().items()}
    net.load_state_dict(sd)
    net = net.to(DEV).train()
    net.set_train_precision(precision)
    return net, sd


def test_fp16_train_step_matches_reference_fp32_and_autocast_goldens(pkg):
    g = np.load(os.path.join(GOLDEN, "train_step.npz"))
    ga = np.load(os.path.join(GOLDEN, "train_step_autocast.npz"))
    net, sd = _net(pkg, 5, "fp16")
    x = torch.from_numpy(pkg.synth.synth_images(2, 128, 128, seed=1))
    hms, tags = net(x.to(DEV))
    assert hms[0].dtype == hms[1].dtype == tags.dtype == torch.float32
    loss = (hms[0] ** 2).mean() + (hms[1] ** 2).mean() + (tags ** 2).mean()
    # loss scale 1024: 32 x below the 32768 at which the reference's own fp16 step is finite, so a few per cent of difference cannot
    # cross 65504; the gradients are unscaled afterwards
    SCALE = 1024.0
    (loss * SCALE).backward()
    params = dict(net.named_parameters())
    for n, p in params.items():
        assert p.grad is not None and torch.isfinite(p.grad).all(), f"{n}: non-finite gradient at loss scale {SCALE}"
        p.grad.div_(SCALE)
    dl, dla = abs(loss.item() - float(g["loss"])) / float(g["loss"]), abs(loss.item() - float(ga["loss"])) / float(ga["loss"])
    ratios_out = []
    for name, t in (("hm0", hms[0]), ("hm1", hms[1]), ("tags", tags)):
        a = t.detach().float().cpu().numpy().ravel()[g[f"{name}.idx"]]
        e_eng = np.sqrt(((a - g[f"{name}.val"]) ** 2).mean())
        e_ref16 = np.sqrt(((ga[f"{name}.val"] - g[f"{name}.val"]) ** 2).mean())
        ratios_out.append(float(e_eng / e_ref16))
    names = [str(n) for n in ga["grad.names"]]
    assert set(names) == set(params)
    nr = np.array([params[n].grad.double().norm().item() / max(ga["grad.norms"][i], 1e-30) for i, n in enumerate(names)])
    # full gradients of the fp32 oracle (autograd on the CPU)
    osd = {k: (v.clone().float().requires_grad_() if k in params else v.clone()) for k, v in sd.items()}
    oh, ot = ofw.higher_hrnet(x, osd, K, train=True)
    ((oh[0] ** 2).mean() + (oh[1] ** 2).mean() + (ot ** 2).mean()).backward()
    cos = []
    for n in names:
        a, b = params[n].grad.float().cpu().flatten(), osd[n].grad.flatten()
        cos.append(float(torch.dot(a, b) / (a.norm() * b.norm() + 1e-30)))
    print(f"fp16 train step: loss rel {dl:.5f} (fp32 golden) {dla:.5f} (autocast golden); rms deviation from fp32, engine fp16 / reference fp16-autocast "
          f"(hm0, hm1, tags): {[round(r, 2) for r in ratios_out]}; grad norm ratio vs autocast [{nr.min():.3f}, {nr.max():.3f}] median {np.median(nr):.3f}; "
          f"cosine vs fp32 oracle min {min(cos):.4f} ({names[int(np.argmin(cos))]}) median {np.median(cos):.4f}")
    assert dl < 5e-3 and dla < 5e-3, (dl, dla)
    assert np.all((nr > 0.75) & (nr < 1.33)) and abs(np.median(nr) - 1) < 0.05, (nr.min(), nr.max(), np.median(nr))
    assert min(cos) > 0.85 and np.median(cos) > 0.95, (min(cos), np.median(cos))
    # one significand bit is a factor 2; a bf16 tensor left anywhere on the path costs three.  Not measured yet
    assert max(ratios_out) < 2.0, ratios_out


# ---------------------------------------------------------------------------------------------------------------- KeypointsModule
B, S = 2, 128


def _module(pkg, precision, seed=0, **kw):
    km = importlib.import_module(PKG + ".keypoints.model")
    net = pkg.HigherHRNet(K, 32)
    net.load_state_dict({k: torch.from_numpy(pkg.synth.synth_param(k, v.shape, seed)) for k, v in net.state_dict().items()})
    model = km.KeypointsModel(net)
    model.to_CUDA(0)
    model.net.train()
    return km.KeypointsModule(model, pkg.AEKeypointsLoss(), torch.optim.Adam(model.net.parameters(), lr=1e-3), precision=precision, **kw)


@pytest.fixture(scope="module")
def batch(pkg):
    """the target construction of test_training_loop_reduces_the_loss, at batch 2"""
    x = torch.from_numpy(pkg.synth.synth_images(B, S, S, 0))
    hms, masks, joints = pkg.synth.synth_train_targets(B, K, S, 3, seed=0)
    return (x.to(DEV), [torch.from_numpy(h).to(DEV) for h in hms], [torch.from_numpy(m).to(DEV) for m in masks], joints)


KEYS = {"loss", "hm_0_loss", "hm_1_loss", "push_0_loss", "pull_0_loss"}


def _params(module):
    return {n: p.detach().clone() for n, p in module.model.net.named_parameters()}


def test_fp16_module_three_steps(pkg, batch):
    module = _module(pkg, "fp16")
    assert module.model.net.train_precision == "fp16" and set(module.scalers) == {"optim"}
    assert type(module.scalers["optim"]) is torch.amp.GradScaler and module.scalers["optim"].get_scale() == 65536.0
    before = _params(module)
    metrics = [module.training_step(batch, i) for i in range(3)]
    for m in metrics:
        assert set(m) == KEYS and all(np.isfinite(v) for v in m.values()), m
        assert abs(m["loss"] - sum(v for k, v in m.items() if k != "loss")) < 1e-4 * abs(m["loss"]) + 1e-6  # the unscaled values
    scale = module.scalers["optim"].get_scale()
    print("fp16 module: losses", [round(m["loss"], 4) for m in metrics], "scale after three steps", scale)
    assert scale in (65536.0, 32768.0, 16384.0, 8192.0), scale
    after = _params(module)
    moved = sum(not torch.equal(before[n], after[n]) for n in before)
    assert moved == len(before), f"{moved} of {len(before)} parameters moved"
    assert all(torch.isfinite(p).all() for p in after.values())
    # the validation step of a net in .train() mode runs the same fp16 forward
    vm, results = module.validation_step(batch)
    assert set(vm) == KEYS and all(np.isfinite(v) for v in vm.values()) and len(results) == B


def test_fp16_module_skips_the_step_at_an_oversized_scale(pkg, batch):
    module = _module(pkg, "fp16")
    module.scalers["optim"] = torch.amp.GradScaler("cuda", init_scale=2.0 ** 40)
    before = _params(module)
    m = module.training_step(batch, 0)
    assert set(m) == KEYS and np.isfinite(m["loss"]) and 0 < m["loss"] < 1e4, m  # still the finite unscaled value
    after = _params(module)
    for n in before:
        assert torch.equal(before[n], after[n]), f"{n} changed in a skipped step"
    steps = [float(st["step"]) for st in module.optimizer.state.values() if "step" in st]
    assert all(s == 0 for s in steps), steps  # (Adam creates its state at the first step it takes: none yet)
    assert module.scalers["optim"].get_scale() == 2.0 ** 39


def test_fp16_module_scaler_state_round_trips(pkg, batch):
    module = _module(pkg, "fp16")
    module.scalers["optim"] = torch.amp.GradScaler("cuda", init_scale=2.0 ** 40)
    module.training_step(batch, 0)  # one skipped step: scale 2^39, growth tracker 0
    module.training_step(batch, 1)
    state = module.state_dict()
    assert set(state) == {"scalers"} and set(state["scalers"]) == {"optim"}
    assert set(state["scalers"]["optim"]) == set(torch.amp.GradScaler("cuda").state_dict())
    fresh = _module(pkg, "fp16", seed=1)
    assert fresh.scalers["optim"].get_scale() == 65536.0
    fresh.load_state_dict(state)
    a, b = module.scalers["optim"], fresh.scalers["optim"]
    assert a.get_scale() == b.get_scale() == state["scalers"]["optim"]["scale"] and a.get_scale() < 2.0 ** 40
    assert a._get_growth_tracker() == b._get_growth_tracker() == state["scalers"]["optim"]["_growth_tracker"]
    assert b.state_dict() == state["scalers"]["optim"]


def test_bf16_module_is_the_step_it_was(pkg, batch):
    """precision="bf16" (the default): no scaler, and one step gives the bits of the sequence training_step ran before the precision
    switch existed (forward, loss, zero_grad, backward, optimizer step), on a second net from the same seed"""
    module = _module(pkg, "bf16")
    assert module.scalers == {} and module.state_dict() == {"scalers": {}} and module.model.net.train_precision == "bf16"
    assert _module(pkg, "fp16").model.net.train_precision == "fp16" and module.precision == "bf16"
    m = module.training_step(batch, 0)
    plain = _module(pkg, "bf16")  # same seed; its training_step is not used
    images, heatmaps, masks, joints = batch
    stages_hms, tags = plain.model.net(images)
    assert stages_hms[0].dtype == torch.float32
    hm_losses, push_losses, pull_losses = plain.loss_fn.calculate_loss(stages_hms, tags, heatmaps, masks, joints)
    loss = 0
    for hl in hm_losses:
        loss = loss + hl
    loss = loss + push_losses[0] + pull_losses[0]
    plain.optimizer.zero_grad()
    loss.backward()
    plain.optimizer.step()
    assert m["loss"] == loss.detach().item()
    for (n, a), (_, b) in zip(module.model.net.named_parameters(), plain.model.net.named_parameters()):
        assert torch.equal(a, b), n
