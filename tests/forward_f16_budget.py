"""Per-tensor error budgets for the fp16 forward (HH_DTYPE_F16 handles), derived from the reference alone: forward_budget.py with the
storage format changed.  A plain module, no tests.

The emulation is oracle/forward.py's storage walk (BatchNorm folded, weights and every stored tensor rounded, sums in fp32) with its
rounding function `_q` replaced, for the duration of one call, by fp32 -> fp16 -> fp32 (torch's conversion: nearest even, subnormals
kept, +-inf beyond +-65504: the semantics of the engine's stores).  The patch is undone in a `finally`; test_forward_f16_budget_cpu.py
holds that the oracle's "fp32" and "bf16" walks give their old bits afterwards.

budget_f16 = MARGIN_F16 x the emulation's five figures (forward_budget.figures / check; TOL_MAX / TOL_RMS stay as caps and do not bind:
the fp16 figures are an eighth of the bf16 ones).

MARGIN_F16 is measured, not taken over: measure_margin_f16() (python tests/forward_f16_budget.py) repeats forward_budget.measure_margin
on the fp16 emulation -- seeds 0..5 (weights and images), 1x64x64 and 2x128x128, W32, every tap and output, per (shape, tensor,
figure) the largest ratio between two seeds' values.  Measured here:
  max x2.65 (stages.3.blocks.0#2 at 1x64x64: 0.00106 .. 0.00280)     rms x1.91 (tags at 2x128x128: 0.00087 .. 0.00166)
  row x1.88 (tags at 2x128x128: 0.00103 .. 0.00193)   col x1.95 (the same: 0.00101 .. 0.00197)   img x1.90 (the same: 0.00088 .. 0.00167)
Rule, as for bf16: the measured scatter rounded up to the next half -> 3.0 for `max`, 2.0 for the other four.

What separates the formats (test_forward_f16_budget_cpu.py): over the nine LATTICE_F16 cases the bf16 emulation exceeds the fp16 budget
in every figure of every output, by at least x3.84 (rms), x3.77 (row), x3.65 (col), x3.77 (img), x2.11 (max).

Worst engine / budget ratio seen on the MI355X (tests/test_gpu_forward_f16.py prints them; profiles/forward_f16.md):
  outputs, nine shapes: max 0.43 (hm_q at 2x128x128), rms 0.50, row 0.53, col 0.54 (hm_h at 1x32x544), img 0.51; logits 0.48
  taps, 1x64x64 and 4x32x32 (worst tap of the group; max / rms / row / col / img):
    stem 0.33 0.50 0.50 0.50 0.50     stages.0 0.46 0.48 0.51 0.48 0.48     stages.1 0.48 0.51 0.53 0.53 0.52
    stages.2 0.57 0.53 0.58 0.58 0.57     stages.3 0.67 0.55 0.61 0.63 0.61     deconv 0.34 0.50 0.48 0.48 0.50
i.e. the engine's error is 1.0x (stem) to 1.2x (stages 2, 3) the emulation's, as for bf16: no rounding that the emulation does not have.
"""
from __future__ import annotations

import functools

import torch

import forward_budget as fb
from oracle import forward as ofw

MARGIN_F16 = {"max": 3.0, "rms": 2.0, "row": 2.0, "col": 2.0, "img": 2.0}  # measured, see the docstring

# (kind, C, B, H, W): the smallest shapes that reach every kernel family and layout.  No 512^2 case: the tile geometry does not depend on
# the element type and tests/test_gpu_forward_lattice.py holds it.
LATTICE_F16 = [
    ("pose", 32, 3, 64, 64),     # 16-row maps: the smallest map the tall layout of the fused block takes
    ("pose", 32, 5, 32, 256),    # 8-row maps, tiles span images
    ("pose", 32, 2, 224, 96),    # 56 rows = 4 exact tiles
    ("pose", 32, 1, 32, 544),    # ragged columns
    ("pose", 32, 4, 32, 32),
    ("pose", 48, 3, 64, 96),     # generic conv widths (KC = 16 families, no fused 32 / 64-channel blocks)
    ("cls", 32, 2, 64, 96),
    ("cls", 32, 4, 32, 32),
    ("pose", 32, 2, 128, 128),
]
OUTPUTS = {"pose": ("hm_q", "hm_h", "tags"), "cls": ("logits",)}


def case_id(case) -> str:
    return "{}{}-{}x{}x{}".format(*case)


def seeds(case):
    i = LATTICE_F16.index(case)
    return 1 + i % 3, 60 + i  # weights, images


def _q_f16(x):
    """fp32 -> fp16 -> fp32: nearest even, subnormals kept, +-inf beyond +-65504"""
    return x.to(torch.float16).to(torch.float32)


def forward_f16(x, sd, classifier: bool = False) -> dict:
    """the fp16-storage emulation: oracle/forward.py's bf16-storage walk with `_q` rounding to fp16 for the duration of this call"""
    saved = ofw._q
    ofw._q = _q_f16
    try:
        return fb._forward(x, sd, "bf16", classifier)  # ("bf16" selects the storage walk: folded BatchNorm, _q at every stored tensor)
    finally:
        ofw._q = saved


@functools.lru_cache(maxsize=12)
def tensors_f16(shape, C: int, seed: int, image_seed: int | None = None, classifier: bool = False):
    """-> (fp32 oracle, fp16-storage emulation): {tap or output name: array}.  Cached: computed once, shared, not to be written to."""
    sd, x = fb.state_dict(C, seed, classifier), fb.images(tuple(shape), seed if image_seed is None else image_seed)
    return fb._forward(x, sd, "fp32", classifier), forward_f16(x, sd, classifier)


def allowed_f16(emulated: dict) -> dict:
    cap = {"max": fb.TOL_MAX, "rms": fb.TOL_RMS}
    return {k: min(MARGIN_F16[k] * emulated[k][0], cap.get(k, float("inf"))) for k in fb.FIGURES}


def budget_f16(tap: str, shape, C: int, seed: int, image_seed: int | None = None, classifier: bool = False) -> dict:
    """allowed figures for tensor `tap` of an fp16 forward (arguments as forward_budget.budget)"""
    ref, emu = tensors_f16(tuple(shape), C, seed, image_seed, classifier)
    return allowed_f16(fb.figures(emu[tap], ref[tap]))


def measure_margin_f16(seeds_=(0, 1, 2, 3, 4, 5), shapes=((1, 64, 64), (2, 128, 128)), C: int = 32):
    """forward_budget.measure_margin on the fp16 emulation: -> {figure: (largest max/min ratio over shapes and tensors, where)}"""
    worst = {k: (1.0, "") for k in fb.FIGURES}
    for shape in shapes:
        per_seed = []
        for s in seeds_:
            sd, x = fb.state_dict(C, s), fb.images(shape, s)
            ref, emu = fb._forward(x, sd, "fp32", False), forward_f16(x, sd)
            per_seed.append({t: fb.figures(emu[t], ref[t]) for t in ref})
        for t in per_seed[0]:
            for k in fb.FIGURES:
                v = [f[t][k][0] for f in per_seed]
                if min(v) > 0 and max(v) / min(v) > worst[k][0]:
                    worst[k] = (max(v) / min(v), f"{t} at {shape}: {min(v):.5f} .. {max(v):.5f}")
    return worst


if __name__ == "__main__":
    torch.set_num_threads(16)
    for k, (ratio, where) in measure_margin_f16().items():
        print(f"{k}: x{ratio:.2f}  ({where})")
