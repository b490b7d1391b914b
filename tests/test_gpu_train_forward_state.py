"""-m gpu: the lifetime of a training forward's state (keypoints/train_net.py: TrainForward).  The packed weights, the SyncBatchNorm
answer and the pending running statistics belong to one forward; nothing of them is left for a later call, another net or a forward
that raised.  Every net is HigherHRNet(5, 32) on synth weights with synth_images(2, 64, 64) in bf16: the smallest input for which every
branch still has more than one sample per channel."""
import importlib

import pytest
import torch
from torch import nn

from conftest import PKG

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED_A, SEED_B = 5, 6
_REF = {}  # seed -> _state of a fresh net after one forward + backward (computed once, read only)


def _mods():
    return importlib.import_module(PKG + ".keypoints.train_net"), importlib.import_module(PKG + ".keypoints.train_ops")


def _net(pkg, seed):
    net = pkg.HigherHRNet(5, 32)
    net.load_state_dict({k: torch.from_numpy(pkg.synth.synth_param(k, v.shape, seed)) for k, v in net.state_dict().items()})
    return net.to(DEV).train()


def _images(pkg, seed):
    return torch.from_numpy(pkg.synth.synth_images(2, 64, 64, seed=seed)).to(DEV)


def _loss(net, x):
    hms, tags = net(x)
    return (hms[0] ** 2).mean() + (hms[1] ** 2).mean() + (tags ** 2).mean()


def _state(net, loss):
    out = {"loss": loss.detach().clone()}
    out.update({"grad " + n: p.grad.clone() for n, p in net.named_parameters()})
    out.update({"buffer " + n: b.clone() for n, b in net.named_buffers()})
    return out


def _step(net, x):
    loss = _loss(net, x)
    loss.backward()
    return _state(net, loss)


def _reference(pkg, seed):
    if seed not in _REF:
        _REF[seed] = _step(_net(pkg, seed), _images(pkg, seed))
    return _REF[seed]


def _assert_same_bits(got, ref, what):
    assert got.keys() == ref.keys()
    bad = [k for k in ref if not torch.equal(got[k], ref[k])]
    assert not bad, f"{what}: {len(bad)} of {len(ref)} tensors differ, first {bad[:3]}"


def test_standalone_conv_does_not_see_a_finished_forwards_packing(pkg):
    """After a forward + backward, a weight of the net changes (as an optimizer step changes it); train_net.conv on that module must
    compute with the weight as it is now.  Before the forward state had an owner this failed: the packed table of the last forward
    stayed at module level, and the stand-alone call picked up the previous packing of this weight."""
    tn, ops = _mods()
    net = _net(pkg, SEED_A)
    _loss(net, _images(pkg, SEED_A)).backward()
    m = net.deconv_layers._modules["0"].resid_blocks._modules["0"].conv1
    assert tuple(m.weight.shape) == (32, 32, 3, 3)
    with torch.no_grad():
        m.weight.mul_(0.5)
    x = torch.randn(1, 32, 6, 16, generator=torch.Generator().manual_seed(1)).to(DEV, torch.bfloat16).contiguous(memory_format=torch.channels_last)
    got, ref = tn.conv(x, m), ops.conv2d(x, m.weight.detach())
    assert ref.float().abs().max().item() > 0
    assert got.shape == ref.shape and torch.equal(got.detach(), ref)


def test_forward_packs_once_and_uses_what_it_packed(pkg, monkeypatch):
    """One forward + backward: PackedConvWeights.refresh runs once; every conv2d call on a weight of the net that the kernels take
    unpadded (cin and cout multiples of 16, 1x1 or 3x3) carries its packed copy, forward and data gradient; the calls on padded copies
    (stem conv1, the two heads at K = 5, the four 2x2 deconv phases) carry none."""
    _, ops = _mods()
    net = _net(pkg, SEED_A)
    x = _images(pkg, SEED_A)
    own = {m.weight.data_ptr() for m in net.modules() if isinstance(m, nn.Conv2d)
           and m.weight.shape[0] % 16 == 0 and m.weight.shape[1] % 16 == 0 and m.weight.shape[2] in (1, 3)}
    calls, refreshes = [], []
    real_conv2d, real_refresh = ops.conv2d, ops.PackedConvWeights.refresh

    def conv2d(*args, **kw):
        calls.append((args[1].data_ptr() in own, bool(kw.get("data_grad", False)), kw.get("packed") is not None))
        return real_conv2d(*args, **kw)

    def refresh(self):
        refreshes.append(self)
        return real_refresh(self)

    monkeypatch.setattr(ops, "conv2d", conv2d)
    monkeypatch.setattr(ops.PackedConvWeights, "refresh", refresh)
    _loss(net, x).backward()
    assert len(refreshes) == 1
    for data_grad in (False, True):
        mine = [packed for is_own, dg, packed in calls if is_own and dg == data_grad]
        assert mine and all(mine), (data_grad, len(mine), sum(mine))
    padded = [(dg, packed) for is_own, dg, packed in calls if not is_own]
    assert not any(packed for _, packed in padded)
    # stem conv1 + 2 heads + 4 deconv phases; the stem's input needs no gradient
    assert sum(not dg for dg, _ in padded) == 7 and sum(dg for dg, _ in padded) == 6


def test_interleaved_forwards_of_two_nets(pkg):
    """forward A, forward B, backward A, backward B == forward A, backward A, forward B, backward B on fresh copies, bit for bit."""
    a, b = _net(pkg, SEED_A), _net(pkg, SEED_B)
    la = _loss(a, _images(pkg, SEED_A))
    lb = _loss(b, _images(pkg, SEED_B))
    la.backward()
    lb.backward()
    _assert_same_bits(_state(a, la), _reference(pkg, SEED_A), "net A")
    _assert_same_bits(_state(b, lb), _reference(pkg, SEED_B), "net B")


def test_forward_that_raises_leaves_nothing_behind(pkg, monkeypatch):
    """A host-side exception in the middle of the forward (the first fusion sum) propagates, updates no running statistic and no
    num_batches_tracked, and the next forward + backward of the same net gives the bits of a fresh identical net."""
    _, ops = _mods()
    net = _net(pkg, SEED_A)
    x = _images(pkg, SEED_A)
    before = {n: b.clone() for n, b in net.named_buffers()}
    assert any("running_mean" in n for n in before) and any("num_batches_tracked" in n for n in before)

    def broken(*args, **kw):
        raise RuntimeError("fusion_sum: broken on purpose")

    with monkeypatch.context() as mp:
        mp.setattr(ops, "fusion_sum", broken)
        with pytest.raises(RuntimeError, match="broken on purpose"):
            net(x)
    changed = [n for n, b in net.named_buffers() if not torch.equal(b, before[n])]
    assert not changed, changed[:3]
    _assert_same_bits(_step(net, x), _reference(pkg, SEED_A), "after the failed forward")
