"""References, error budgets and a numpy model of the gradient statistics and the global-norm clip (csrc/grad_stats.hip,
csrc/grad_stats_math.h, optim.clip_grad_norm_); a plain module like optim_budget.py, shared by test_grad_clip_cpu.py and
test_gpu_grad_clip.py.

Reference: fp64 (numpy's pairwise sums) from the fp32 gradients.
    l2 = sqrt(sum g^2), absmax = max |g|, absmean = sum |g| / n per tensor; total_l2 = sqrt(sum over all elements of g^2),
    total_inf = max over the tensors of absmax.
Budget: from the operands and u = 2^-24 alone; nothing here comes from a kernel's output.  The kernels form g^2 in fp64, where the
product of two fp32 values is exact, and add n of them in fp64: off by at most n 2^-53 of the sum (every term >= 0).  The reference's
own sum is off by no more than that.  sqrt and the division by n are one fp64 rounding each (2^-53, inside the n 2^-53 for n >= 1
counted twice), and the ONE rounding that shows is the last, to fp32: u |x|.  So
    allowed(l2)      = (u + 2 n 2^-53) l2  + 2^-150        (the last term: half the smallest subnormal, for a norm that underflows)
    allowed(absmean) = (u + 2 n 2^-53) absmean + 2^-150
    allowed(total)   = (u + 2 N 2^-53) total + 2^-150,  N = all elements
    absmax, total_inf, the non-finite count: exact (a maximum and an integer), allowed = 0
That is half an fp32 ulp at the top of a binade and one at its bottom: the fp64-accumulating rule lands on the correctly rounded value
or next to it.  torch's own clip_grad_norm_ accumulates in fp32 and is 88-114 ulp away on random gradients of this lattice (printed by
the CPU test, in units of this budget), which is why no budget is taken from torch.
Clip: coef is torch's fp32 expression of the RETURNED total, max_norm / (total + 1e-6) clamped to at most 1, and the gradients are
g0 * coef in fp32: both bit for bit, no budget.
"""
import numpy as np

U = 2.0 ** -24
F = np.float32
CHUNK, THREADS, WAVE = 4096, 256, 64

SIZES = [1, 7, 8, 17, 255, 256, 257, 4096, 4097, 65539, 589824, 4096 * 257 + 3]
GRAD_SCALES = (1e-6, 1e-3, 1.0, 30.0)
OFFSETS = (0, 1, 3)  # tensor k's gradient sits k % 3 -> this many elements past a 16-byte boundary (1, 3: the scalar path)


def lattice_grads(seed=0, mul=1.0):
    """one fp32 gradient per SIZES entry; tensor k at gradient scale GRAD_SCALES[k % 4]"""
    rng = np.random.default_rng(seed)
    return [(rng.standard_normal(n) * GRAD_SCALES[k % 4]).astype(F) * F(mul) for k, n in enumerate(SIZES)]


def constant_grads(n=589824, c=0.7):
    """one tensor of n elements +-c with alternating signs: one magnitude, so that every rounding of a low-precision chain errs in the
    same direction (what averages out on random gradients adds up here)"""
    return [np.where(np.arange(n) % 2, F(-c), F(c)).astype(F)]


def exact_grads():
    """0 / +-1 with 4^j non-zeros per tensor (the largest power of 4 that fits), one of them the last element: every partial sum is an
    integer below 2^24, so every summation order, in fp32 or fp64, is exact.  Sum of squares over SIZES: 1 385 049."""
    out = []
    for n in SIZES:
        nz = 1
        while nz * 4 <= n:
            nz *= 4
        g = np.zeros(n, dtype=F)
        if nz > 1:
            pos = np.arange(nz - 1) * ((n - 1) // (nz - 1))
            g[pos] = np.where(np.arange(nz - 1) % 2, F(-1), F(1))
        g[n - 1] = 1
        assert np.count_nonzero(g) == nz
        out.append(g)
    return out


# ---- reference and budget
def reference(grads):
    """-> rows [n, 4] fp64 (l2, absmax, absmean, non-finite count), total_l2, total_inf"""
    rows = np.zeros((len(grads), 4))
    ss_total = 0.0
    with np.errstate(invalid="ignore", over="ignore"):
        for k, g in enumerate(grads):
            if g.size == 0:
                continue
            d = g.astype(np.float64)
            ss = np.sum(d * d)
            rows[k] = (np.sqrt(ss), np.max(np.abs(d)), np.sum(np.abs(d)) / g.size, np.count_nonzero(~np.isfinite(d)))
            ss_total += ss
        return rows, float(np.sqrt(ss_total)), float(np.max(rows[:, 1])) if len(grads) else 0.0


def budget(grads):
    """-> allowed |error| of the rows [n, 4] and of total_l2 (total_inf: 0)"""
    rows, total, _ = reference(grads)
    n = np.array([g.size for g in grads], dtype=np.float64)
    rel = U + 2 * n * 2.0 ** -53
    allowed = np.zeros_like(rows)
    allowed[:, 0] = rel * rows[:, 0] + 2.0 ** -150
    allowed[:, 2] = rel * rows[:, 2] + 2.0 ** -150
    return allowed, (U + 2 * n.sum() * 2.0 ** -53) * total + 2.0 ** -150


def clip_coef(max_norm, total):
    """torch's fp32 arithmetic: max_norm / (total + 1e-6), clamped to at most 1 (a NaN stays)"""
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        c = F(max_norm) / (F(total) + F(1e-6))
    return F(1.0) if c > F(1.0) else c


def worst(got, ref, allowed):
    """max |got - ref| / allowed (an exact result counts as 0, also inside a zero budget; any error against a zero budget as inf)"""
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / allowed)
    return float(np.max(r)) if r.size else 0.0


# ---- a numpy model of the kernels' own order (grad_stats_math.h), and of planted defects
def _thread_values(g, aligned):
    """[chunks, THREADS, 17] fp32: the values thread t of each chunk's workgroup accumulates, in its order, zero-padded (adding +0 to
    a sum of non-negative terms changes nothing), and the mask of real entries"""
    n = g.size
    nch = (n + CHUNK - 1) // CHUNK
    pad = np.zeros(nch * CHUNK, dtype=F)
    pad[:n] = g
    valid = np.zeros(nch * CHUNK, dtype=bool)
    valid[:n] = True
    vals = np.zeros((nch, THREADS, 17), dtype=F)
    mask = np.zeros((nch, THREADS, 17), dtype=bool)
    for c in range(nch):
        m = min(CHUNK, n - c * CHUNK)
        ch, va = pad[c * CHUNK:(c + 1) * CHUNK], valid[c * CHUNK:(c + 1) * CHUNK]
        if aligned:
            done = m // 4 * 4
            in4 = va & (np.arange(CHUNK) < done)
            # element (it * THREADS + t) * 4 + j  ->  thread t, position it * 4 + j
            vals[c, :, :16] = np.where(in4, ch, F(0)).reshape(4, THREADS, 4).transpose(1, 0, 2).reshape(THREADS, 16)
            mask[c, :, :16] = in4.reshape(4, THREADS, 4).transpose(1, 0, 2).reshape(THREADS, 16)
            tail = m - done  # elements done + t, t < tail <= 3
            vals[c, :tail, 16] = ch[done:m]
            mask[c, :tail, 16] = True
        else:  # element t + THREADS * k -> thread t, position k
            vals[c, :, :16] = ch.reshape(16, THREADS).T
            mask[c, :, :16] = va.reshape(16, THREADS).T
    return vals, mask


def _max_nan(a, b):
    """grad_max_nan: keeps a NaN (np.maximum does)"""
    with np.errstate(invalid="ignore"):
        return np.maximum(a, b)


def _block_reduce(ss, sa, mx, cnt, drop_nan=False):
    """[..., THREADS] -> [...]: lane i += lane i + off for off = 32 .. 1 in each wave, then (w0 + w1) + (w2 + w3)"""
    fmax = np.fmax if drop_nan else _max_nan
    sh = ss.shape[:-1] + (THREADS // WAVE, WAVE)
    ss, sa, mx, cnt = ss.reshape(sh).copy(), sa.reshape(sh).copy(), mx.reshape(sh).copy(), cnt.reshape(sh).copy()
    off = WAVE // 2
    with np.errstate(invalid="ignore", over="ignore"):
        while off:
            ss[..., :off] = ss[..., :off] + ss[..., off:2 * off]
            sa[..., :off] = sa[..., :off] + sa[..., off:2 * off]
            mx[..., :off] = fmax(mx[..., :off], mx[..., off:2 * off])
            cnt[..., :off] = cnt[..., :off] + cnt[..., off:2 * off]
            off //= 2
        w = lambda a, op: op(op(a[..., 0, 0], a[..., 1, 0]), op(a[..., 2, 0], a[..., 3, 0]))  # noqa: E731
        add = lambda x, y: x + y  # noqa: E731
        return w(ss, add), w(sa, add), w(mx, fmax), w(cnt, add)


def _strided_share(a, op, zero):
    """[n] -> [THREADS]: thread t combines entries t, t + THREADS, ... in that order, from `zero`"""
    rounds = (len(a) + THREADS - 1) // THREADS
    padded = np.full(rounds * THREADS, zero, dtype=a.dtype)
    padded[:len(a)] = a
    acc = np.full(THREADS, zero, dtype=a.dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(rounds):
            acc = op(acc, padded[r * THREADS:(r + 1) * THREADS])
    return acc


def model_stats(grads, offsets=None, inv_scale=None, defect=None):
    """The kernels in numpy, operation by operation and in their order: -> dict(rows [n, 4] fp32, total_l2, total_inf (fp32),
    found_inf, grads (the stored gradients: g * inv_scale where inv_scale is given and not 1)).
    defect: "fp32_accumulate" (squares and sums in fp32), "drop_nan" (fmaxf's maximum), "stats_of_scaled" (the fused pass takes the
    statistics of the value it read, not of the one it stores)."""
    acc_t = F if defect == "fp32_accumulate" else np.float64
    drop = defect == "drop_nan"
    fmax = np.fmax if drop else _max_nan
    rows = np.zeros((len(grads), 4), dtype=F)
    tss, stored, found = np.zeros(len(grads), dtype=acc_t), [], False
    for k, g in enumerate(grads):
        g = np.asarray(g, dtype=F)
        found = found or bool((~np.isfinite(g)).any())
        with np.errstate(invalid="ignore", over="ignore"):
            out = g * F(inv_scale) if inv_scale is not None and F(inv_scale) != F(1) else g
        stored.append(out)
        if g.size == 0:
            continue
        src = g if defect == "stats_of_scaled" else out
        vals, mask = _thread_values(src, aligned=(offsets[k] if offsets is not None else OFFSETS[k % 3]) % 4 == 0)
        ss, sa = np.zeros(vals.shape[:2], dtype=acc_t), np.zeros(vals.shape[:2], dtype=acc_t)
        mx, cnt = np.zeros(vals.shape[:2], dtype=F), np.zeros(vals.shape[:2], dtype=np.int64)
        with np.errstate(invalid="ignore", over="ignore"):
            for j in range(17):  # one thread's elements in the order of its walk
                d = vals[..., j].astype(acc_t)
                ss = ss + d * d
                sa = sa + np.abs(d)
                mx = fmax(mx, np.abs(vals[..., j]))
                cnt = cnt + (mask[..., j] & ~np.isfinite(vals[..., j]))
        pss, psa, pmx, pcnt = _block_reduce(ss, sa, mx, cnt, drop)  # one record per chunk
        add = lambda x, y: x + y  # noqa: E731
        t = _block_reduce(_strided_share(pss, add, acc_t(0)), _strided_share(psa, add, acc_t(0)), _strided_share(pmx, fmax, F(0)),
                          _strided_share(pcnt, add, np.int64(0)), drop)
        tss[k] = t[0]
        with np.errstate(invalid="ignore"):
            if np.isnan(t[2]):
                rows[k] = (np.nan, np.nan, np.nan, t[3])
            else:
                rows[k] = (F(np.sqrt(t[0])), t[2], F(t[1] / acc_t(g.size)), t[3])
    add = lambda x, y: x + y  # noqa: E731
    z = np.zeros(THREADS)
    tot = _block_reduce(_strided_share(tss, add, acc_t(0)), z.astype(acc_t), _strided_share(rows[:, 1].copy(), fmax, F(0)), z.astype(np.int64), drop)
    with np.errstate(invalid="ignore"):
        nan = bool(np.isnan(tot[2]))
        total_l2 = F(np.nan) if nan else F(np.sqrt(tot[0]))
        total_inf = F(np.nan) if nan else F(tot[2])
    return dict(rows=rows, total_l2=total_l2, total_inf=total_inf, found_inf=found, grads=stored)


def model_clip(stats, max_norm, norm_type=2.0, found_inf=False, defect=None):
    """-> (coef fp32, the gradients after the scale pass).  defect: "no_eps", "no_clamp", "per_tensor" (each tensor by its own norm),
    "ignore_found_inf" (the scale pass runs although the flag is set)."""
    inf = norm_type == float("inf")
    total = stats["total_inf"] if inf else stats["total_l2"]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        def coef_of(t):
            c = F(max_norm) / (F(t) if defect == "no_eps" else F(t) + F(1e-6))
            return c if defect == "no_clamp" or not c > F(1) else F(1)
        coef = coef_of(total)
        if found_inf and defect != "ignore_found_inf":
            return coef, [g.copy() for g in stats["grads"]]
        out = []
        for k, g in enumerate(stats["grads"]):
            c = coef_of(stats["rows"][k, 1 if inf else 0]) if defect == "per_tensor" else coef
            out.append(g.copy() if c >= F(1) and defect != "no_clamp" else g * c)
    return coef, out
