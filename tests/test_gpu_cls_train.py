"""-m gpu: ClassificationHRNet in .train() mode on the HIP training kernels (bf16 activations; fp32 parameters, pooled features, Linear and
loss) against the reference's own training step (tests/golden/cls_train_step.npz: the reference net in .train() mode, its
ClassificationLoss, torch autograd; tools/make_golden.py cls_train) and against the fp32 oracle's full gradients; then the running
statistics, an optimizer step followed by an eval forward, the trainer-facing module, and DistributedDataParallel.

The bounds of the end-to-end comparison are the project's own for the same kernels at the same statistics
(test_gpu_parity.py::test_train_step_batch8_matches_reference_autograd_tightly: 8 images of 128 x 128, so the lowest-resolution branch
normalises over 128 samples per channel): loss within 0.3 %, logits within 4 % of max, every parameter's gradient norm within 10 % (median
within 2 %), cosine against the oracle's gradient > 0.92 (median > 0.98).

Two of them do not hold for this net and loss, and not because of the kernels: the per-parameter norm ratio and the cosine.  A CPU
emulation that never touches the engine (tests/cls_emulation.py: torch fp32 with every conv / BatchNorm / sum output, and the gradient
with respect to it, rounded to bf16) sits this far from the same golden and oracle:
    emulation: norm ratio [0.745, 1.224] median 0.9959, cosine min 0.758 median 0.9035 (loss 0.011 %, logits 3.1 % of max)
    engine:    norm ratio [0.747, 1.269] median 0.9954, cosine min 0.730 median 0.900  (loss 0.009 %, logits 2.8 % of max; MI355X)
Those two bounds are therefore 1.5 x the emulation's own deviation (tests/test_cls_emulation_cpu.py holds the recorded figures):
    norm ratio in (1 - 1.5 x 0.255, 1 + 1.5 x 0.224) = (0.6175, 1.336);  cosine min > 1 - 1.5 x 0.242 = 0.637, median > 1 - 1.5 x 0.0965 = 0.855
The loss, logit and median-ratio bounds stay as they are.  The four conv biases in front of a train-mode BatchNorm
(classification_head.downsample_blocks.{0,1,2}.0.bias, final_conv.0.bias) are left out of the ratio and cosine checks: their true gradient
is zero and the reference's is rounding noise (test_cls_budget_cpu.py holds the golden's below 1e-3 of the following BatchNorm's dbeta);
the engine's is asserted below the same fraction here.
"""
import functools
import importlib
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cls_emulation as ce
from conftest import GOLDEN, PKG
from oracle import forward as ofw

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED_W, SEED_X = ce.SEED_W, ce.SEED_X
_E = ce.EMULATION_DEVIATION  # see the module docstring
RATIO_LO, RATIO_HI = 1 - 1.5 * (1 - _E["ratio_min"]), 1 + 1.5 * (_E["ratio_max"] - 1)
COS_MIN, COS_MEDIAN = 1 - 1.5 * (1 - _E["cos_min"]), 1 - 1.5 * (1 - _E["cos_median"])
HEAD = "classification_head."
SILENT_BIASES = {HEAD + f"downsample_blocks.{i}.0.bias": HEAD + f"downsample_blocks.{i}.1.bias" for i in range(3)}
SILENT_BIASES[HEAD + "final_conv.0.bias"] = HEAD + "final_conv.1.bias"


def _golden():
    return np.load(os.path.join(GOLDEN, "cls_train_step.npz"))


def _synth_sd(pkg, net, seed=SEED_W):
    return {k: torch.from_numpy(pkg.synth.synth_param(k, v.shape, seed)) for k, v in net.state_dict().items()}


def _make(pkg, seed=SEED_W):
    net = pkg.ClassificationHRNet(32, 1000)
    net.load_state_dict(_synth_sd(pkg, net, seed))
    return net.to(DEV).train()


@functools.lru_cache(maxsize=None)
def _engine_step():
    """one training forward + backward of the engine on the golden's inputs -> (net, logits, loss, metrics); shared, left unchanged"""
    pkg = importlib.import_module(PKG)
    loss_mod = importlib.import_module(PKG + ".classification.loss")
    g = _golden()
    net = _make(pkg)
    x = torch.from_numpy(pkg.synth.synth_images(8, 128, 128, seed=SEED_X)).to(DEV)
    logits = net(x)
    fn = loss_mod.ClassificationLoss()
    loss = fn.calculate_loss(torch.from_numpy(g["targets"]).to(DEV), logits)
    loss.backward()
    return net, logits.detach().cpu(), loss.item(), fn.metrics()


@functools.lru_cache(maxsize=None)
def _oracle_grads():
    """the fp32 oracle (oracle.forward._classification_hrnet with its train flag set) + torch autograd on the CPU -> {name: gradient}"""
    pkg = importlib.import_module(PKG)
    g = _golden()
    net = pkg.ClassificationHRNet(32, 1000)
    sd = _synth_sd(pkg, net)
    pnames = {n for n, _ in net.named_parameters()}
    osd = {k: (v.clone().float().requires_grad_() if k in pnames else v.clone()) for k, v in sd.items()}
    x = torch.from_numpy(pkg.synth.synth_images(8, 128, 128, seed=SEED_X))
    ofw._TRAIN = True
    try:
        logits = ofw._classification_hrnet(x, osd)
    finally:
        ofw._TRAIN = False
    F.cross_entropy(logits, torch.from_numpy(g["targets"])).backward()
    return {k: osd[k].grad for k in pnames}, logits.detach()


def test_train_forward_backward_matches_reference_autograd(pkg):
    """(a) of the module docstring."""
    g = _golden()
    net, logits, loss, metrics = _engine_step()
    assert logits.shape == (8, 1000) and logits.dtype == torch.float32
    dl = abs(loss - float(g["loss"])) / float(g["loss"])
    el = float(np.abs(logits.numpy() - g["logits"]).max() / np.abs(g["logits"]).max())
    ograds, ologits = _oracle_grads()
    assert float(np.abs(ologits.numpy() - g["logits"]).max()) < 1e-4 * np.abs(g["logits"]).max()  # the oracle is the reference's forward
    names = [str(n) for n in g["grad.names"]]
    # the golden's four gradient samples per parameter tie the oracle's full gradients to the reference's autograd (two fp32 CPU runs of
    # the same graph: agreement to 1e-3 of the parameter's largest gradient; measured worst 5e-7.  The four silent biases are left out: theirs is noise)
    for i, n in enumerate(names):
        if n in SILENT_BIASES:
            continue
        og = ograds[n].flatten()
        idx = np.linspace(0, og.numel() - 1, 4).astype(int)
        assert np.abs(og[idx].numpy() - g["grad.samples"][i]).max() <= 1e-3 * float(og.abs().max()) + 1e-12, n
    params = dict(net.named_parameters())
    assert set(names) == set(params) and all(p.grad is not None for p in params.values())
    gnorm = dict(zip(names, g["grad.norms"]))
    checked = [n for n in names if n not in SILENT_BIASES]
    ratios = np.array([params[n].grad.double().norm().item() / max(gnorm[n], 1e-30) for n in checked])
    cos = np.array([float(torch.dot(params[n].grad.float().cpu().flatten(), ograds[n].flatten()) /
                          (params[n].grad.float().cpu().norm() * ograds[n].norm() + 1e-30)) for n in checked])
    print(f"cls train step B=8: loss rel {dl:.5f}, logits max err / absmax {el:.4f}, grad norm ratio [{ratios.min():.3f} ({checked[int(ratios.argmin())]}), "
          f"{ratios.max():.3f} ({checked[int(ratios.argmax())]})] median {np.median(ratios):.4f}, cosine min {cos.min():.4f} ({checked[int(cos.argmin())]}) "
          f"median {np.median(cos):.4f}; metrics {metrics}")
    for b, bn_bias in SILENT_BIASES.items():
        ours = params[b].grad.double().norm().item()
        print(f"  {b}: engine gradient norm {ours:.3g}, golden {gnorm[b]:.3g}, dbeta norm {params[bn_bias].grad.double().norm().item():.3g}")
        assert ours < 1e-3 * params[bn_bias].grad.double().norm().item(), b
    assert dl < 3e-3 and el < 4e-2, (dl, el)
    assert np.all((ratios > RATIO_LO) & (ratios < RATIO_HI)) and abs(np.median(ratios) - 1) < 0.02, (ratios.min(), ratios.max(), np.median(ratios))
    assert cos.min() > COS_MIN and np.median(cos) > COS_MEDIAN, (cos.min(), np.median(cos))
    # the hit counts: no row of the fixture can flip within the logit bound (test_cls_budget_cpu.py), so they are the golden's
    assert metrics["top-1_error"] == float(g["top-1_error"]) and metrics["top-5_error"] == float(g["top-5_error"])
    assert metrics["loss"] == loss


def test_running_statistics_match_the_reference(pkg):
    """(b) After one training forward the running statistics are 0.9 x the loaded value + 0.1 x the batch statistic (unbiased variance).
    The issue asks for equality with the golden to fp32 rounding of the batch statistics.  bf16 activations cannot give that: the batch
    statistics are taken over tensors that were stored in bf16, layers deep.  The tolerance is therefore derived as for (a): the
    bf16-storage emulation of tests/cls_emulation.py, which never touches the engine, records the same three statistics, and the engine
    may sit 1.5 x as far from the golden as that emulation does (max |difference| over the channels; EMULATION_STAT_DISTANCE, held by
    tests/test_cls_emulation_cpu.py):
        statistic                                                      emulation   bound (1.5 x)   engine (MI355X)
        backbone.bn1.running_mean                                      6.26e-6     9.39e-6         6.26e-6
        classification_head.downsample_blocks.0.1.running_mean         5.49e-4     8.24e-4         6.57e-4
        classification_head.final_conv.1.running_var                   1.082e-2    1.623e-2        9.73e-3
    downsample_blocks.0.1.running_mean holds the conv bias, which no kernel adds to the activations: it enters through the recorded batch
    mean, and leaving it out would miss by 0.1 x |bias| (up to 0.032)."""
    g = _golden()
    net = _engine_step()[0]
    st = net.state_dict()
    keys = [k[5:] for k in g.files if k.startswith("stat.")]
    assert sorted(keys) == sorted(ce.EMULATION_STAT_DISTANCE)
    dist = {k: float(np.abs(st[k].cpu().numpy() - g["stat." + k]).max()) for k in keys}
    for k in keys:
        print(f"{k}: engine max |diff| {dist[k]:.4g}, emulation {ce.EMULATION_STAT_DISTANCE[k]:.4g}, bound {1.5 * ce.EMULATION_STAT_DISTANCE[k]:.4g}")
    for k in keys:
        assert dist[k] <= 1.5 * ce.EMULATION_STAT_DISTANCE[k], (k, dist[k], ce.EMULATION_STAT_DISTANCE[k])
    assert int(st["backbone.bn1.num_batches_tracked"]) == int(st[HEAD + "final_conv.1.num_batches_tracked"]) == 1
    k = HEAD + "downsample_blocks.0.1.running_mean"
    bias = st[HEAD + "downsample_blocks.0.0.bias"].cpu().numpy()
    without = float(np.abs(st[k].cpu().numpy() - 0.1 * bias - g["stat." + k]).max())
    print(f"running_mean without the conv bias: max |diff| {without:.4g} (0.1 |bias| up to {0.1 * np.abs(bias).max():.3g})")
    assert without > 1.5 * ce.EMULATION_STAT_DISTANCE[k]


def test_one_optimizer_step_then_eval(pkg):
    """(c) One SGD(nesterov) step on the gradients of a training forward, then an eval forward on the engine: the updated weights and
    running statistics are re-folded, the logits are finite and differ from those before the step."""
    net = _make(pkg)
    x = torch.from_numpy(pkg.synth.synth_images(2, 64, 64, seed=3)).to(DEV)
    net.eval()
    with torch.no_grad():
        before = net(x).clone()
    net.train()
    opt = torch.optim.SGD(net.parameters(), lr=0.05, momentum=0.9, nesterov=True)
    loss_mod = importlib.import_module(PKG + ".classification.loss")
    loss = loss_mod.ClassificationLoss().calculate_loss(torch.tensor([1, 2], device=DEV), net(x))
    loss.backward()
    w0 = net.classification_head.classifier.weight.detach().clone()
    opt.step()
    assert not torch.equal(w0, net.classification_head.classifier.weight)
    net.eval()
    with torch.no_grad():
        after = net(x)
    assert after.shape == before.shape == (2, 1000) and torch.isfinite(after).all() and not torch.equal(after, before)


def test_module_training_and_validation_steps(pkg):
    """(d) ClassificationModule on 4 images of 64 x 64 (the reference's initialisation, SGD with Nesterov momentum at lr 0.01): the
    loss of a fixed batch falls over 10 steps; validation_step returns the three metrics and one record per image."""
    cls = importlib.import_module(PKG + ".classification")
    torch.manual_seed(0)
    model = cls.ClassificationModel(pkg.ClassificationHRNet(32, 1000))
    model.init_weights()
    model.to_CUDA(0)
    model.net.train()
    opt = torch.optim.SGD(model.net.parameters(), lr=0.01, momentum=0.9, nesterov=True)
    module = cls.ClassificationModule(model, cls.ClassificationLoss(), opt)
    batch = module.batch_to_device((torch.from_numpy(pkg.synth.synth_images(4, 64, 64, seed=2)), torch.tensor([3, 141, 592, 653])))
    losses = []
    for step in range(10):
        m = module.training_step(batch, step)
        assert set(m) == {"loss", "top-1_error", "top-5_error"} and np.isfinite(m["loss"])
        losses.append(m["loss"])
    print("ClassificationModule losses over 10 steps:", [round(v, 4) for v in losses])
    assert losses[-1] < losses[0]
    metrics, results = module.validation_step(batch, 0)
    assert set(metrics) == {"loss", "top-1_error", "top-5_error"} and np.isfinite(metrics["loss"]) and 0.0 <= metrics["top-5_error"] <= metrics["top-1_error"] <= 1.0
    assert len(results) == 4 and model.net.training
    for r, t in zip(results, [3, 141, 592, 653]):
        assert r.logits.shape == (1000,) and r.target == t and r.prediction == int(np.argmax(r.logits))
    assert metrics["top-1_error"] == 1 - sum(r.prediction == r.target for r in results) / 4


def test_training_step_with_a_bad_target_raises_before_any_weight_moves(pkg):
    cls = importlib.import_module(PKG + ".classification")
    model = cls.ClassificationModel(_make(pkg, 5))
    opt = torch.optim.SGD(model.net.parameters(), lr=0.1, momentum=0.9, nesterov=True)
    module = cls.ClassificationModule(model, cls.ClassificationLoss(), opt)
    before = {n: p.detach().clone() for n, p in model.net.named_parameters()}
    batch = module.batch_to_device((torch.from_numpy(pkg.synth.synth_images(2, 64, 64, seed=2)), torch.tensor([3, 1000])))
    with pytest.raises(IndexError):
        module.training_step(batch, 0)
    assert all(torch.equal(before[n], p) for n, p in model.net.named_parameters()) and not opt.state


def test_train_step_under_distributed_data_parallel(pkg):
    """(e) One rank on RCCL: the gradients DistributedDataParallel reduces equal the plain module's bit for bit (every parameter takes
    part in the graph, the four silent conv biases included)."""
    import torch.distributed as dist
    cls = importlib.import_module(PKG + ".classification")
    x = torch.from_numpy(pkg.synth.synth_images(2, 64, 64, seed=2)).to(DEV)
    t = torch.tensor([5, 7], device=DEV)

    def grads(m):
        cls.ClassificationLoss().calculate_loss(t, m(x)).backward()
    plain = _make(pkg, 5)
    grads(plain)
    created = not dist.is_initialized()
    if created:
        dist.init_process_group("nccl", init_method="tcp://127.0.0.1:29547", rank=0, world_size=1, device_id=torch.device(DEV))
    try:
        model = cls.ClassificationModel(_make(pkg, 5))
        model.to_DDP(0, use_batchnorm=False)
        grads(model.net)
        torch.cuda.synchronize()
        for (n, a), (_, b) in zip(plain.named_parameters(), model.net.module.named_parameters()):
            assert b.grad is not None and torch.equal(a.grad, b.grad), n
    finally:
        if created:
            dist.destroy_process_group()
