"""Shared by tests/test_train_input_cpu.py, tests/test_gpu_train_input.py and tools/make_train_input_golden.py: the golden
fixture of the training input, its seeded raw samples, and the recorder of the global RNG draws."""
import hashlib
import importlib
import json
import os
import random

import numpy as np
import pytest

from conftest import GOLDEN, PKG


@pytest.fixture(scope="module")
def ti_mod():
    return importlib.import_module(PKG + ".keypoints.train_input")


@pytest.fixture(scope="module")
def golden():
    return json.load(open(os.path.join(GOLDEN, "train_input_meta.json"))), np.load(os.path.join(GOLDEN, "train_input.npz"))


def golden_sample(pkg, meta, case):
    img, mask, joints = pkg.synth.synth_train_sample(case["h"], case["w"], case["people"], case["sample_seed"], meta["num_kpts"], case["holes"])
    assert hashlib.sha256(img.tobytes() + mask.tobytes() + joints.tobytes()).hexdigest() == case["sha256"], "the seeded raw sample changed"
    return img, mask, joints


def golden_transform(ti_mod, meta, case, **kw):
    tf = dict(meta["transform"], scale_type="long" if case["mode"] == "train_long" else meta["transform"]["scale_type"])
    ti = ti_mod.TrainInput(meta["out_size"], meta["hm_resolutions"], num_kpts=meta["num_kpts"], sigma=meta["sigma"], **tf, **kw)
    return ti, (ti.inference if case["mode"] == "inference" else ti.train)


class Recorder:
    """Wraps the three global RNG entry points the transform draws from and lists (name, value) in call order."""

    def __enter__(self):
        self.draws, self.saved = [], (np.random.random, np.random.randint, random.random)

        def wrap(fn, name):
            def f(*a, **k):
                v = fn(*a, **k)
                self.draws.append([name, float(v)])
                return v
            return f
        np.random.random, np.random.randint, random.random = (wrap(self.saved[0], "np.random.random"), wrap(self.saved[1], "np.random.randint"),
                                                              wrap(self.saved[2], "random.random"))
        return self

    def __exit__(self, *exc):
        np.random.random, np.random.randint, random.random = self.saved


def golden_draw(mode, case):
    """Seeds both global RNGs as the fixture did and draws: -> (AugParams, the list of draws made)."""
    np.random.seed(case["rng_seed"])
    random.seed(case["rng_seed"])
    with Recorder() as rec:
        p = mode.draw(case["h"], case["w"])
    return p, rec.draws
