"""-m gpu: the fused stem in its producer / consumer form (csrc/stem_fused.hip) stores, bit for bit, the words the one-group form of
the parent commit stored: tests/golden/stem_bits.npz, recorded from that commit's kernel by tools/make_stem_golden.py, which also
defines the shapes, the seeds and how the words are obtained (hh_debug_stem_fused: the stem alone, so that partial tiles and ragged
widths run, which hh_forward's multiples of 32 never reach)."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, REPO

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("make_stem_golden", os.path.join(REPO, "tools", "make_stem_golden.py"))
msg = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(msg)


@pytest.fixture(scope="module")
def golden():
    g = np.load(os.path.join(GOLDEN, "stem_bits.npz"))
    meta = json.loads(str(g["meta"]))
    assert len(meta["parent_commit"]) == 40 and [tuple(s) for s in meta["shapes"]] == msg.SHAPES
    assert (meta["weight_seed"], meta["image_seed"]) == (msg.WEIGHT_SEED, msg.IMAGE_SEED)
    return g


@pytest.fixture(scope="module")
def nets(pkg):
    return {dtype: msg.make_net(pkg, dtype) for dtype in msg.DTYPES}


def _same_words(got, g, k):
    """`got` against what the golden file keeps under k: all words, or their digests and the strided sample (make_stem_golden.record)."""
    if k + "/words" in g.files:
        want = g[k + "/words"]
        assert got.shape == want.shape and got.dtype == want.dtype == np.uint16, k
        d = got != want
        assert not d.any(), f"{k}: {int(d.sum())} of {d.size} words differ, first at {tuple(np.argwhere(d)[0])}"
        return
    want = g[k + "/sample"]
    sample = got[msg.SAMPLE]
    assert sample.shape == want.shape and sample.dtype == want.dtype == np.uint16, k
    assert np.array_equal(sample, want), f"{k}: {int((sample != want).sum())} of {want.size} sampled words differ"
    per_image = [msg.digest(w) for w in got]
    bad = [i for i, (a, b) in enumerate(zip(per_image, g[k + "/image_sha256"].tolist())) if a != b]
    assert not bad and len(per_image) == len(g[k + "/image_sha256"]), f"{k}: images {bad} differ"
    assert msg.digest(got) == str(g[k + "/sha256"]), k


@pytest.mark.parametrize("dtype", msg.DTYPES)
@pytest.mark.parametrize("i", range(len(msg.SHAPES)), ids=[msg.key("", s)[1:] for s in msg.SHAPES])
def test_stem_words_equal_the_parent_kernels(pkg, golden, nets, dtype, i):
    got = msg.stem_words(pkg, nets[dtype], msg.images(pkg, i))
    assert not (got == 0xFFFF).any(), "a word of the output was not written"
    _same_words(got, golden, msg.key(dtype, msg.SHAPES[i]))


@pytest.mark.parametrize("dtype", msg.DTYPES)
def test_stem_words_do_not_depend_on_stale_lds(pkg, golden, dtype):
    """The largest shape (every workgroup walks 2 or 3 tiles through both LDS buffers) with NaN patterns in every CU's LDS in front
    of the launch (HH_POISON_LDS=1): the same bits."""
    i = len(msg.SHAPES) - 1
    net = msg.make_net(pkg, dtype, {"HH_POISON_LDS": "1"})
    _same_words(msg.stem_words(pkg, net, msg.images(pkg, i)), golden, msg.key(dtype, msg.SHAPES[i]))


@pytest.mark.parametrize("i", (4, 5), ids=[msg.key("", msg.SHAPES[i])[1:] for i in (4, 5)])
def test_two_launch_stem_within_tolerance(pkg, nets, i):
    """HH_NO_STEM_FUSED=1 (stem_conv.hip + a conv launch, the second implementation) on the two shapes hh_forward accepts: the stem#0 tap
    of the two plans within the tolerance of test_fused_stem_matches_two_launches (4e-2 of the maximum, 2e-2 rms), and the fused
    plan's tap is the stand-alone entry's words."""
    x = msg.images(pkg, i)
    taps = []
    for net in (nets["bf16"], msg.make_net(pkg, "bf16", {"HH_NO_STEM_FUSED": "1"})):
        net.set_taps(True)
        net.forward_raw(x)
        torch.cuda.synchronize()
        taps.append(net.read_taps()["stem#0"])
        net.set_taps(False)
    one, two = (torch.from_numpy(t) for t in taps)
    assert (one - two).abs().max().item() <= 4e-2 * two.abs().max().item()
    assert (one - two).pow(2).mean().sqrt().item() <= 2e-2 * two.pow(2).mean().sqrt().item()
    words = msg.stem_words(pkg, nets["bf16"], x)  # [B, h, w, 64] bf16 words -> fp32 NCHW, exactly
    as_f32 = (words.astype(np.uint32) << 16).view(np.float32).transpose(0, 3, 1, 2)
    assert np.array_equal(as_f32, taps[0])
