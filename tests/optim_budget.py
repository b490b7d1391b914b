"""References and error budgets of the device optimizer step (csrc/optim.hip, pytorch-human-pose_amd/optim.py); a plain module like
train_budget.py, shared by test_optim_budget_cpu.py and test_gpu_optim.py.

Reference: the update in fp64 (numpy, or torch on the CPU for net-sized checks) from the fp32 operands and the double hyper-parameters.
Budget: from the operands and u = 2^-24 alone, every operation taken on absolute values; nothing here comes from a kernel's output.

Adam / AdamW, with G = |g| + wd |p| (AdamW: G = |g|) and primes for the fp64 results:
  m' = m + (1 - b1)(g - m): the difference, the product with the rounded 1 - b1 and the sum, each on values <= |m| + G
        A_m = 4 u (|m| + G)
  v' = b2 v + (1 - b2) g^2: two rounded constants, the square, two products and the sum; G enters squared, so its 3 u doubles
        A_v = 8 u (b2 v + (1 - b2) G^2)
  sqrt:  e_sqrt = sqrt(v' + A_v) - sqrt(v')   (exact for any v', no derivative at 0)
  D = sqrt(v') / sqrt(bc2) + eps: the rounded sqrt(bc2), the division, the rounded eps and the sum
        e_D = e_sqrt / sqrt(bc2) + 3 u D
  U = (lr / bc1) m' / D:  e_U = (lr / bc1)(A_m / D + |m'| e_D / D^2) + 3 u |U|   (the rounded step size, the division, the product)
  allowed(p') = u |p'| + e_U  (+ 2 u |p| for AdamW: the rounded 1 - lr wd and the product)
  allowed(m') = A_m + u |m'|,  allowed(v') = A_v + u |v'|
SGD (dampening 0), with g2 = g + wd p, b' = mu b + g2, d = g2 + mu b' (Nesterov), b' (plain) or g2 (mu = 0):
  g2: the rounded wd, the product and the sum                 A_g = 3 u G            (0 when wd = 0: g2 = g exactly)
  b': the rounded mu, the product, the sum, on top of A_g      A_b = A_g + 3 u (mu |b| + G)
  d (Nesterov): A_g + mu A_b + the rounded mu, the product and the sum on values <= G + mu |b'|
                                                              A_d = A_g + mu A_b + 3 u (G + mu |b'|)
  p' = p - lr d: the rounded lr, the product, the sum          allowed(p') = u |p'| + lr (A_d + 2 u |d|)
  allowed(b') = A_b
Step counters: exact (step + 1 on an applied step, unchanged on a skipped one).
"""
import numpy as np

U = 2.0 ** -24
F = np.float32


def _f64(*a):
    """numpy arrays or torch CPU tensors (the module-sized checks: torch's fp64 arithmetic runs on all cores), as fp64"""
    return [x.double() if hasattr(x, "double") else np.asarray(x, dtype=np.float64) for x in a]


def _sqrt(x):
    return x ** 0.5  # (both libraries take the square-root path for this exponent)


def adam_reference(p, g, m, v, step, lr, b1, b2, eps, wd, decoupled):
    """-> p', m', v' in fp64; `step` is the number of this step (the counter before it, plus one)."""
    p, g, m, v = _f64(p, g, m, v)
    if wd != 0:
        if decoupled:
            p = p * (1.0 - lr * wd)
        else:
            g = g + wd * p
    m2 = m + (1.0 - b1) * (g - m)
    v2 = b2 * v + (1.0 - b2) * g * g
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    return p - (lr / bc1) * m2 / (_sqrt(v2) / _sqrt(bc2) + eps), m2, v2


def adam_budget(p, g, m, v, step, lr, b1, b2, eps, wd, decoupled):
    """-> allowed |error| of p', m', v'."""
    p, g, m, v = _f64(p, g, m, v)
    p2, m2, v2 = adam_reference(p, g, m, v, step, lr, b1, b2, eps, wd, decoupled)
    G = abs(g) + (0.0 if decoupled else wd * abs(p))
    A_m = 4 * U * (abs(m) + G)
    A_v = 8 * U * (b2 * v + (1.0 - b2) * G * G)
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    e_sqrt = _sqrt(v2 + A_v) - _sqrt(v2)
    D = _sqrt(v2) / _sqrt(bc2) + eps
    e_D = e_sqrt / _sqrt(bc2) + 3 * U * D
    Uabs = (lr / bc1) * abs(m2) / D
    e_U = (lr / bc1) * (A_m / D + abs(m2) * e_D / (D * D)) + 3 * U * Uabs
    allowed_p = U * abs(p2) + e_U + (2 * U * abs(p) if decoupled and wd != 0 else 0.0)
    return allowed_p, A_m + U * abs(m2), A_v + U * abs(v2)


def sgd_reference(p, g, buf, lr, wd, mu, nesterov):
    """-> p', buf' in fp64 (buf' is None for mu = 0); a fresh momentum buffer is zeros (dampening 0: the first step gives buf = g)."""
    p, g = _f64(p, g)
    if wd != 0:
        g = g + wd * p
    b2 = None
    if mu != 0:
        b2 = mu * _f64(buf)[0] + g
        g = g + mu * b2 if nesterov else b2
    return p - lr * g, b2


def sgd_budget(p, g, buf, lr, wd, mu, nesterov):
    """-> allowed |error| of p', buf' (None for mu = 0)."""
    p, g = _f64(p, g)
    p2, b2 = sgd_reference(p, g, buf, lr, wd, mu, nesterov)
    G = abs(g) + wd * abs(p)
    A_g = 3 * U * G if wd != 0 else G * 0.0
    g2 = g + wd * p
    if mu == 0:
        A_d, d, A_b = A_g, g2, None
    else:
        A_b = A_g + 3 * U * (mu * abs(_f64(buf)[0]) + G)
        if nesterov:
            A_d = A_g + mu * A_b + 3 * U * (G + mu * abs(b2))
            d = g2 + mu * b2
        else:
            A_d, d = A_b, b2
    return U * abs(p2) + lr * (A_d + 2 * U * abs(d)), A_b


# ---- the same updates op by op in fp32 (numpy rounds every operation): a model of a correct kernel, and of planted defects
def adam_fp32(p, g, m, v, step, lr, b1, b2, eps, wd, decoupled, defect=None):
    p, g, m, v = [np.asarray(x, dtype=F) for x in (p, g, m, v)]
    if defect == "swap_decay":  # L2 applied as decoupled decay and the reverse
        decoupled = not decoupled
    if wd != 0:
        if decoupled:
            p = p * F(1.0 - lr * wd)
        else:
            g = g + F(wd) * p
    fb1, fb2 = (float(F(b1)), float(F(b2))) if defect == "fp32_betas" else (b1, b2)
    m2 = m + F(1.0 - fb1) * (g - m)
    v2 = F(fb2) * v + F(1.0 - fb2) * (g * g)
    bc1, bc2 = 1.0 - fb1 ** step, 1.0 - fb2 ** step
    if defect == "no_bias_correction":
        bc1 = bc2 = 1.0
    if defect == "eps_in_root":
        denom = np.sqrt(v2 + F(eps)) / F(np.sqrt(bc2))
    else:
        denom = np.sqrt(v2) / F(np.sqrt(bc2)) + F(eps)
    return p - F(lr / bc1) * (m2 / denom), m2, v2


def sgd_fp32(p, g, buf, lr, wd, mu, nesterov, defect=None):
    p, g = np.asarray(p, dtype=F), np.asarray(g, dtype=F)
    if defect == "plain_momentum":
        nesterov = False
    if wd != 0:
        g = g + F(wd) * p
    b2 = None
    if mu != 0:
        b2 = F(mu) * np.asarray(buf, dtype=F) + g
        g = g + F(mu) * b2 if nesterov else b2
    return p - F(lr) * g, b2


# ---- the CPU lattice: steps x gradient scales x weight decay, 20 000 elements per case
STEPS = (1, 2, 10, 1000, 100000)
GRAD_SCALES = (1e-6, 1e-3, 1.0, 30.0)
WDS = (0.0, 1e-2)
N = 20000


def operands(seed, gscale, step, n=N):
    """fp32 p, g, m, v of a plausible state after `step - 1` steps at this gradient scale: m ~ bc1 * g-sized, v ~ bc2 * g^2-sized,
    with a tenth of the elements at a 100 x smaller gradient than their history and a tenth at zero gradient."""
    rng = np.random.default_rng(seed)
    p = (rng.standard_normal(n) * np.exp(rng.uniform(-4, 1, n))).astype(F)
    g = (rng.standard_normal(n) * gscale).astype(F)
    k = rng.random(n)
    g[k < 0.1] *= F(0.01)
    g[k > 0.9] = 0
    prev = step - 1
    bc1, bc2 = 1 - 0.9 ** prev, 1 - 0.999 ** prev
    m = (rng.standard_normal(n) * gscale * bc1).astype(F)
    v = ((rng.standard_normal(n) * gscale) ** 2 * bc2).astype(F)
    return p, g, m, v


def worst(got, ref, allowed):
    """max |got - ref| / allowed (0 / 0 counts as 0: an exact result inside a zero budget)."""
    if hasattr(ref, "double"):  # torch
        import torch
        err = (got.double() - ref).abs()
        return float(torch.where(err == 0, torch.zeros_like(err), err / allowed).max()) if err.numel() else 0.0
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / allowed)
    return float(np.max(r)) if r.size else 0.0
