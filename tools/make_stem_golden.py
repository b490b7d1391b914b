#!/usr/bin/env python3
"""tests/golden/stem_bits.npz: the raw 16-bit words the fused stem (csrc/stem_fused.hip) stores, recorded ONCE on the GPU from the
library of the commit whose kernel a rewrite must reproduce bit for bit (tests/test_gpu_stem_pc.py):

    HH_LIB=/path/to/parent/libhhrnet.so python tools/make_stem_golden.py --parent <commit> [--out tests/golden/stem_bits.npz]

The parent library needs hh_debug_stem_fused (include/hhrnet.h), the stem-alone entry: four of the six shapes are no multiples of
32 and never pass hh_forward.  For a parent commit older than that entry, build its stem_fused.hip into this tree's library.

Per element type (bf16, fp16) one HigherHRNet(17, 32) with synth weights of seed WEIGHT_SEED; per shape i synth images of seed
IMAGE_SEED + i.  A shape of at most FULL_WORDS words is kept whole ("<dtype>/<B>x<H>x<W>/words", uint16 [B, H/4, W/4, 64]).  The
largest shape has 2.2 M words per element type, 4.5 MB each, over the size a committed file may have: of it the file keeps the
sha256 of all words, one sha256 per image (to say WHERE a mismatch is) and every word at [:, ::8, ::8, ::4] -- equal digests are
equal words.  This module is also the test's only definition of the shapes, the seeds and the way the words are obtained."""
import argparse
import contextlib
import hashlib
import importlib
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "pytorch-human-pose_amd"
# (B, H, W): one partial tile; one exact tile; partial last row tile + a second column tile one pixel wide; ragged width; narrow map;
# 544 tiles on 256 workgroups (2 and 3 tiles per workgroup, consecutive tiles of one workgroup in different images, prologue and drain)
SHAPES = [(1, 4, 4), (1, 8, 128), (2, 12, 132), (3, 8, 260), (5, 64, 32), (17, 256, 128)]
DTYPES = ("bf16", "fp16")
WEIGHT_SEED, IMAGE_SEED = 5, 11
FULL_WORDS = 50_000
SAMPLE = (slice(None), slice(None, None, 8), slice(None, None, 8), slice(None, None, 4))


def key(dtype, shape):
    return f"{dtype}/{shape[0]}x{shape[1]}x{shape[2]}"


@contextlib.contextmanager
def switches(env):
    """HH_* plan switches are read once in hh_create: set them around the construction of a net only."""
    os.environ.update(env)
    try:
        yield
    finally:
        for k in env:
            del os.environ[k]


def make_net(pkg, dtype, env=None, C=32):
    import torch
    with switches(env or {}):
        net = pkg.HigherHRNet(17, C, dtype=dtype)
    net.load_state_dict({k: torch.from_numpy(pkg.synth.synth_param(k, v.shape, WEIGHT_SEED)) for k, v in net.state_dict().items()})
    return net.to("cuda:0").eval()


def images(pkg, i):
    import torch
    return torch.from_numpy(pkg.synth.synth_images(*SHAPES[i], IMAGE_SEED + i)).to("cuda:0")


def stem_words(pkg, net, x):
    """The stem's output for images x [B,3,H,W] as stored: uint16 [B, H/4, W/4, 64].  The output buffer starts as 0xFFFF words, which
    the kernel never stores (ReLU), so a word it leaves unwritten cannot pass for one it wrote."""
    import torch
    x = net._check_input(x)  # (packs the weights on first use)
    B, _, H, W = x.shape
    out = torch.full((B, H // 4, W // 4, 64), -1, dtype=torch.int16, device=x.device)
    pkg._lib.launch(x.device, net._lib.hh_debug_stem_fused, net._h, x.data_ptr(), B, H, W, out.data_ptr())
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint16)


def digest(words):
    return hashlib.sha256(np.ascontiguousarray(words).tobytes()).hexdigest()


def record(words):
    """What the file keeps of one shape's words: {"words"} or {"sha256", "image_sha256", "sample"}."""
    if words.size <= FULL_WORDS:
        return {"words": words}
    return {"sha256": np.array(digest(words)), "image_sha256": np.array([digest(w) for w in words]), "sample": np.ascontiguousarray(words[SAMPLE])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True, help="the commit the loaded library's stem kernel is built from")
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "stem_bits.npz"))
    a = ap.parse_args()
    sys.path.insert(0, REPO)
    pkg = importlib.import_module(PKG)
    out = {}
    for dtype in DTYPES:
        net = make_net(pkg, dtype)
        for i, shape in enumerate(SHAPES):
            words = stem_words(pkg, net, images(pkg, i))
            assert not (words == 0xFFFF).any(), (dtype, shape, "unwritten words")
            for k, v in record(words).items():
                out[f"{key(dtype, shape)}/{k}"] = v
            print(key(dtype, shape), words.shape, digest(words)[:16], f"{(words == 0).mean():.2f} zeros")
    out["meta"] = np.array(json.dumps({"parent_commit": a.parent, "library": os.path.basename(pkg._lib.SO), "weight_seed": WEIGHT_SEED,
                                       "image_seed": IMAGE_SEED, "shapes": SHAPES, "dtypes": DTYPES, "net": "HigherHRNet(17, 32)"}))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    np.savez_compressed(a.out, **out)
    print(a.out, os.path.getsize(a.out), "bytes")


if __name__ == "__main__":
    main()
