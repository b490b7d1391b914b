"""The CPU side of the training forward's state object (keypoints/train_net.py: TrainForward): the running-statistics update it ends
with, the constant its BatchNorm scratch allocations share with the kernels, and that the module keeps no state of its own."""
import importlib
import os
import re

import numpy as np
import pytest
import torch
from torch import nn

from conftest import PKG, REPO


@pytest.mark.parametrize("momenta", [(0.1, 0.1), (0.1, 0.3)])
def test_flush_running_stats_matches_torch_batchnorm(pkg, momenta):
    """TrainForward.pending filled by hand with (module, mean, invstd, count) - computed in float64, rounded to fp32 - then flushed, over
    three steps, against nn.BatchNorm2d in train mode on the same inputs: running_mean, running_var, num_batches_tracked.  Equal momenta
    take the multi-tensor branch, different ones the per-module branch.  Bound: rtol 1e-5, about eight fp32 roundings per step over three
    steps (measured worst relative difference 2.7e-7)."""
    tn = importlib.import_module(PKG + ".keypoints.train_net")
    g = torch.Generator().manual_seed(7)
    layers = [(8, 4, 6), (24, 2, 3)]  # (C, B, hw)
    ours = [nn.BatchNorm2d(C, momentum=mom).train() for (C, _, _), mom in zip(layers, momenta)]
    refs = [nn.BatchNorm2d(C, momentum=mom).train() for (C, _, _), mom in zip(layers, momenta)]
    for step in range(3):
        fw = tn.TrainForward()
        assert fw.sync is None and fw.packed is None and fw.pending == []
        for (C, B, hw), m, ref in zip(layers, ours, refs):
            x = torch.randn(B, C, hw, hw, generator=g) * (1 + step) + 0.3 * step
            ref(x)
            x64 = x.double()
            mean, var = x64.mean((0, 2, 3)), x64.var((0, 2, 3), unbiased=False)
            fw.pending.append((m, mean.float(), (var + m.eps).rsqrt().float(), B * hw * hw))
        fw.flush_running_stats()
        assert fw.pending == []
    for m, ref in zip(ours, refs):
        np.testing.assert_allclose(m.running_mean.numpy(), ref.running_mean.numpy(), rtol=1e-5, atol=0)
        np.testing.assert_allclose(m.running_var.numpy(), ref.running_var.numpy(), rtol=1e-5, atol=0)
        assert int(m.num_batches_tracked) == int(ref.num_batches_tracked) == 3


def test_bn_block_count_matches_the_kernels_and_the_header(pkg):
    ops = importlib.import_module(PKG + ".keypoints.train_ops")
    kernels_h = open(os.path.join(REPO, PKG, "csrc", "kernels.h")).read()
    (blocks,) = re.findall(r"^#define\s+HH_BN_BLOCKS\s+(\d+)", kernels_h, re.M)
    assert ops.BN_BLOCKS == int(blocks)
    stated = re.findall(r"scratch: (\d+) ?\* ?C ?\* ?2 doubles", open(pkg._lib.HEADER).read())
    assert stated and all(int(n) == ops.BN_BLOCKS for n in stated), stated


def test_train_net_keeps_no_module_level_container(pkg):
    tn = importlib.import_module(PKG + ".keypoints.train_net")
    held = [k for k, v in vars(tn).items() if isinstance(v, (list, dict, set)) and not k.startswith("__")]
    assert held == []
