"""Shared by tests/test_train_mosaic_cpu.py, tests/test_gpu_train_mosaic.py and tools/make_train_mosaic_golden.py: the golden fixture
of the mosaic (tests/golden/train_mosaic.npz + train_mosaic_meta.json), its seeded pool of raw samples, and a recorder of the global
RNG draws that also lists random.randint (the draw of the three other tiles, coco.py:305)."""
import hashlib
import json
import os
import random

import numpy as np
import pytest

from conftest import GOLDEN
from train_input_helpers import Recorder


class MosaicRecorder(Recorder):
    """train_input_helpers.Recorder plus random.randint, in call order.  (random.randint draws through getrandbits, not through
    random.random: nothing is listed twice.)"""

    def __enter__(self):
        super().__enter__()
        self.saved_randint = random.randint

        def randint(a, b):
            v = self.saved_randint(a, b)
            self.draws.append(["random.randint", float(v)])
            return v
        random.randint = randint
        return self

    def __exit__(self, *exc):
        random.randint = self.saved_randint
        super().__exit__(*exc)


@pytest.fixture(scope="module")
def mosaic_golden():
    return json.load(open(os.path.join(GOLDEN, "train_mosaic_meta.json"))), np.load(os.path.join(GOLDEN, "train_mosaic.npz"))


def pool_sha(pool) -> str:
    return hashlib.sha256(b"".join(a.tobytes() for s in pool for a in s)).hexdigest()


def make_pool(synth, spec, num_kpts: int, integer: bool):
    """The raw samples behind the fixture: synth.synth_train_sample per [h, w, people, seed, holes]; `integer`: the joints as an int64
    array (COCO's annotations are integers), else float64."""
    pool = [synth.synth_train_sample(h, w, people, seed, num_kpts, holes) for h, w, people, seed, holes in spec]
    return [(img, mask, joints.astype(np.int64) if integer else joints) for img, mask, joints in pool]


def golden_pool(pkg, meta, case):
    pool = make_pool(pkg.synth, meta["pool"], meta["num_kpts"], case["integer_joints"])
    assert pool_sha(pool) == case["pool_sha256"], "the seeded raw samples changed"
    return pool


def canvas_sha(canvas, canvas_mask) -> str:
    return hashlib.sha256(np.ascontiguousarray(canvas).tobytes() + np.ascontiguousarray(canvas_mask).astype(np.uint8).tobytes()).hexdigest()
