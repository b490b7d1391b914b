"""Reference and error budget of the weight EMA (csrc/ema.hip, optim.ModelEMA); a plain module like optim_budget.py, shared by
test_ema_budget_cpu.py and test_gpu_ema.py.

Rule (csrc/ema_math.h), n = the update counter before the update, value = the weights the update sees (the stepped p'):
  skipped step (found_inf):  ema' = ema, the bits kept
  n == 0:                    ema' = value, the bits copied
  otherwise:                 d = min(decay, (1 + n) / (10 + n)) with warm-up, decay without;  w = 1 - d;  ema' = ema + w (value - ema)
Reference: that in fp64 from the fp32 operands and the double decay.

Budget, from the operands and u = 2^-24 alone (nothing here comes from a kernel's output), every operation taken on absolute values:
  the difference value - ema:                      u (|value| + |ema|)
  the product with the once-rounded w:             the difference's error times w, the rounding of w (u w on the difference) and the
                                                   product's own rounding (u on the product): 3 u w (|value| + |ema|) together
  the sum:                                         u |ema'|
      allowed(ema') = (3 u w (|value| + |ema|) + u |ema'|) (1 + 2^-20) + 2^-149
  plus w * allowed(value) where the reference chain starts from an fp64 value that the fp32 one only approximates within
  allowed(value) (optim_budget.py's p'); the GPU tests read the stepped fp32 parameters back and need no such term.
  The copy and the skipped step are exact: allowed = 0 (the copy: allowed(value)).
Second-order terms: the three first-order terms above are u-sized; the dropped products of two roundings are u times smaller, i.e.
2^-24 of the budget, and the sum's rounding acts on the computed sum, which is within the other two terms of |ema'| -- again u times
them.  The factor (1 + 2^-20) covers all of these sixteen-fold (and fp64's own 2^-53 roundings in the reference) without loosening
the first order by more than a millionth; 2^-149 is one fp32 denormal step, for a product that underflows.  So: yes, the factor is
needed for a bound that is a bound, and it is there.  On the CPU lattice below (504 cases of 20 000 elements) an fp32 model of the rule
reaches 0.9998 of the budget: the sum's term u |ema'| has no slack where the average sits just above a power of two.
"""
import numpy as np

from optim_budget import U, F, _f64, worst  # noqa: F401  (worst is this module's ratio too)

SECOND_ORDER = 1.0 + 2.0 ** -20
TINY = 2.0 ** -149


def ema_weight(n, decay, warmup):
    """w = 1 - d in fp64"""
    d = min(decay, (1.0 + n) / (10.0 + n)) if warmup else decay
    return 1.0 - d


def ema_reference(ema, value, n, decay, warmup, found_inf=False):
    """-> ema' in fp64"""
    ema, value = _f64(ema, value)
    if found_inf:
        return ema
    if n == 0:
        return value
    return ema + ema_weight(n, decay, warmup) * (value - ema)


def ema_budget(ema, value, n, decay, warmup, found_inf=False, allowed_value=0.0):
    """-> allowed |error| of ema'"""
    ema, value = _f64(ema, value)
    if found_inf:
        return ema * 0.0
    if n == 0:
        return value * 0.0 + allowed_value
    w = ema_weight(n, decay, warmup)
    ref = ema + w * (value - ema)
    return (3 * U * w * (abs(value) + abs(ema)) + U * abs(ref)) * SECOND_ORDER + TINY + w * allowed_value


# ---- the rule op by op in fp32 (numpy rounds every operation): a model of a correct kernel, and of planted defects
DEFECTS = ("fp32_decay", "counter_after_advance", "no_copy", "old_value", "update_on_skip")


def ema_fp32(ema, value, n, decay, warmup, found_inf=False, defect=None, old_value=None):
    """`old_value`: the weights before the step (what the defect "old_value" averages instead of the stepped ones)."""
    ema, value = np.asarray(ema, dtype=F), np.asarray(value, dtype=F)
    if found_inf and defect != "update_on_skip":
        return ema
    if defect == "old_value":
        value = np.asarray(old_value, dtype=F)
    if defect == "counter_after_advance":  # the counter as the tail launch leaves it
        n = n + 1
    if n == 0 and defect != "no_copy":
        return value.copy()
    if defect == "fp32_decay":
        d = F(decay)
        if warmup:
            d = min(d, F((1.0 + n) / (10.0 + n)))
        w = F(1.0) - d
    else:
        w = F(ema_weight(n, decay, warmup))
    return ema + w * (value - ema)


# ---- the lattices
DECAYS = (0.9998, 0.5, 0.0, 1.0)                         # the GPU lattice's
CPU_DECAYS = (0.0, 2.0 / 11.0, 0.5, 0.9, 0.999, 0.9998, 1.0)
COUNTERS = (0, 1, 7, 10 ** 6)
WARMUPS = (False, True)
MAGNITUDES = (1e-3, 1.0, 1e3)
N = 20000


def operands(seed, ema_mag, value_mag, n=N):
    """fp32 ema, value (the stepped weights) and old value (before the step: 1e-3 of its size away)"""
    rng = np.random.default_rng(seed)
    ema = (rng.standard_normal(n) * ema_mag).astype(F)
    value = (rng.standard_normal(n) * value_mag).astype(F)
    k = rng.random(n)
    value[k < 0.1] = ema[k < 0.1]          # a tenth already at the average: the difference is exactly zero
    value[k > 0.95] = 0
    old = (value * F(1.001) + F(1e-3 * value_mag)).astype(F)
    return ema, value, old


def cpu_cases():
    """(seed, ema magnitude, value magnitude, n, decay, warmup) over the whole CPU lattice"""
    seed = 0
    for em in MAGNITUDES:
        for vm in MAGNITUDES:
            for n in COUNTERS:
                for decay in CPU_DECAYS:
                    for warmup in WARMUPS:
                        seed += 1
                        yield seed, em, vm, n, decay, warmup


# the case each planted defect is named to fail on: (ema magnitude, value magnitude, n, decay, warmup, found_inf)
DEFECT_CASES = {
    "fp32_decay": (1e-3, 4.0, 7, 0.9998, False, False),          # 1 - fl(0.9998) is off by ~1e-4 of w
    "counter_after_advance": (1.0, 1.0, 1, 0.9998, True, False),  # the ramp at n = 1 is 2/11, at n + 1 it is 3/12
    "no_copy": (1.0, 1.0, 0, 0.9998, False, False),               # the average's storage holds anything before the first update
    "old_value": (1.0, 1.0, 7, 0.5, False, False),                # the weights before the step
    "update_on_skip": (1.0, 1.0, 7, 0.5, False, True),            # a skipped step must keep the bits
}
