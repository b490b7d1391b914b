"""References, error budgets and lattices of the training objective (csrc/loss_kernels.hip behind hh_loss_heatmaps and
hh_loss_ae_grouping, wrapped by pytorch-human-pose_amd/keypoints/loss.py); a plain module like train_budget.py and optim_budget.py,
shared by test_loss_budget_cpu.py and test_gpu_loss_lattice.py.

Reference: both losses and every gradient in fp64 (numpy) from the fp32 operands, written from the formulas oracle/loss.py documents.
Budget: from the operands, u = 2^-24 (fp32) and v = 2^-53 (fp64) alone; nothing here comes from a kernel's output.  s = 2^-149 is the
smallest fp32 subnormal.

Masked MSE, N = B K h w, masks in [0, 1]
  gradient   the kernel forms fl(fl(fl(2/N) * fl(p - t)) * m): four roundings               allowed = 4 u |g| + s
             (s: a product that lands in the subnormal range is off by at most s/2, twice)
  loss       every term is fl(fl(d d) m) with d = fl(p - t): 2 u from d, one rounding per product, 4 u on a non-negative term, so
             4 u on the sum; the sum and the division are taken in double (at most N v relative), the cast adds u
                                                                                            allowed = (5 u + N v) loss + 2 s
             (2 s: every term may lose s to underflow, so may their mean; the cast of a subnormal loss, s/2)
  through autograd the stored gradient is multiplied by the incoming one in fp32 (+ u |g|) and cast to the input's dtype (+ half an ulp
  of that dtype, HALF_ULP below).

Grouping loss.  Every operation is in double; the values are cast to fp32 once.  With, per person, n visible joints, tags t_k, mean m,
d_k = t_k - m, and per image `nobj` people that have a visible joint:
  e_m   = (n + 1) v mean|t_k|                 (n - 1 additions and the division, on values <= sum|t_k|)
  e_d   = e_m + v |d_k|
  pull  = mean_b (1/nobj) sum_p (1/n) sum_k d_k^2
        E_pull = mean_b (1/nobj) sum_p (1/n) sum_k (2 |d_k| e_d + (n + 3) v d_k^2) + (P + B + 6) v pull
  push  = mean_b c (sum_{a,q} exp(-(m_a - m_q)^2) - nobj),  c = 0.5 / (nobj (nobj - 1)); D = m_a - m_q, e = exp(-D^2)
        e_D   = e_m[a] + e_m[q] + v |D|
        rel_e = 2 |D| e_D + v D^2 + EXP_REL   (EXP_REL = 4 * 2^-52: the allowance for `exp` in double on either side, documented as
                1 ulp on the device, below 1 ulp in the host's libm, and the rounded argument; the diagonal is exp(-0) = 1 exactly)
        E_push = mean_b c (sum_{a != q} e rel_e + (P + 10) v sum_{a,q} e) + (B + 3) v |push|
  The fp64 reference commits errors of the same size, so both E enter twice:
        allowed(push) = u |push| + 2 E_push + s,   allowed(pull) = u |pull| + 2 E_pull + s
  gradient   one contribution per visible joint, c_i = push_scale/B (dpush/dm)/n + pull_scale/(B nobj) 2 d_k / n, formed in double
             and rounded ONCE to fp32, then added atomically in fp32 onto the map:
        E_i = push_scale/(B n) c (sum_q 4 (e_D e + |D| e rel_e) + (P + 10) v sum_q 4 |D| e) + pull_scale/(B nobj) 2/n (e_m + 6 v |d_k|)
        a pixel with contributions c_1 .. c_h:
        allowed = sum_i (u |c_i| + 2 E_i + s)                                                   (the casts)
                + 0                          h = 1   (0 + c is exact)
                + u |sum c_i| + u^2 sum|c_i| h = 2   (one rounding of the sum of the two rounded values: independent of the order)
                + (h - 1) u sum|c_i|         h >= 3  (h - 1 roundings of partial sums, in an order that changes from run to run)
  through autograd (AEKeypointsLoss multiplies push and pull by 1e-3): the map returned is fl(fl(gpush a) + fl(gpull b)) with
  a, b = the incoming gradients, themselves fl(1e-3 * upstream), two roundings from the exact 0.001 * upstream:
        allowed = |a| allowed(gpush) + |b| allowed(gpull) + 4 u (|gpush a| + |gpull b|)      (+ HALF_ULP of a narrower dtype)

The op-by-op models (`mse_fp32`, `grouping_model`) are what a correct kernel computes, as optim_budget.adam_fp32 is for the optimizer;
`defect=` plants one of MSE_DEFECTS / GROUPING_DEFECTS.  The model must stay inside every budget, every defect must leave it.  The
grouping model is written as the kernel's loops and shares no code with the vectorised reference; it holds the reference's formulas and
the fp32 part of the budget.  Whether the fp64 terms (e_m, e_D, rel_e) are large enough is shown by the run on the MI355X (another
summation order, another `exp`) and by the comparison with oracle/loss.py, not by the model.
"""
import functools
import zlib
from types import SimpleNamespace

import numpy as np

U = 2.0 ** -24
V = 2.0 ** -53
SUB = 2.0 ** -149
EXP_REL = 4 * 2.0 ** -52
F = np.float32
PLANES_PER_LAUNCH = 1024  # HH_LOSS_SCRATCH: the grid of masked_mse_kernel stops growing here
HALF_ULP = {"float32": (U, 2.0 ** -150), "float16": (2.0 ** -11, 2.0 ** -25), "bfloat16": (2.0 ** -8, 2.0 ** -134)}  # relative, floor


def half_ulp(x, dtype):
    """bound of the rounding of x to `dtype` ("float16", "bfloat16")"""
    rel, floor = HALF_ULP[dtype]
    return np.maximum(rel * np.abs(x), floor)


def worst(got, ref, allowed):
    """max |got - ref| / allowed (0 / 0 counts as 0: an exact result inside a zero budget).  A NaN or an inf in `got`, or anything else
    that keeps the ratio from being a number, counts as an infinite error: the result is never NaN."""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        err = np.abs(np.asarray(got, dtype=np.float64) - ref)
        r = np.where(err == 0, 0.0, err / allowed)
    r = np.where(np.isfinite(r), r, np.inf)
    return float(np.max(r)) if r.size else 0.0


# ======================================================================================================================== masked MSE
def mse_reference(pred, target, mask):
    """-> loss (python float), d loss / d pred (fp64 [B,K,h,w])"""
    p, t, m = (np.asarray(a, dtype=np.float64) for a in (pred, target, mask))
    with np.errstate(invalid="ignore", over="ignore"):
        d = p - t
        return float((d * d * m[:, None]).sum() / p.size), 2.0 * d * m[:, None] / p.size


def mse_budget(pred, target, mask):
    """-> allowed |error| of the loss and of every gradient element"""
    loss, g = mse_reference(pred, target, mask)
    return (5 * U + g.size * V) * abs(loss) + 2 * SUB, 4 * U * np.abs(g) + SUB


MSE_DEFECTS = ("mask_per_plane", "N_without_K", "no_factor_2", "tail_dropped", "planes_beyond_grid_dropped")


def mse_fp32(pred, target, mask, defect=None):
    """masked_mse_kernel + sum_partials_kernel op by op (numpy rounds every fp32 operation) -> loss (fp32), gradient (fp32)"""
    p, t, m = (np.asarray(a, dtype=F) for a in (pred, target, mask))
    B, K, h, w = p.shape
    hw = h * w
    n = float(B * h * w if defect == "N_without_K" else B * K * h * w)
    gscale = F((1.0 if defect == "no_factor_2" else 2.0) / n)
    if defect == "mask_per_plane":  # mask + plane * hw where mask + b * hw belongs (wrapped into the buffer)
        mm = m.reshape(B, hw)[np.arange(B * K) % B].reshape(B, K, h, w)
    else:
        mm = np.broadcast_to(m[:, None], p.shape)
    d = p - t
    term = (d * d) * mm
    grad = ((gscale * d) * mm).reshape(B * K, hw).copy()
    keep = np.ones((B * K, hw), bool)
    if defect == "tail_dropped" and hw // 4 > 256:  # only the full trips of the lane loop
        keep[:, hw // 4 // 256 * 256 * 4:] = False
    if defect == "planes_beyond_grid_dropped":
        keep[PLANES_PER_LAUNCH:] = False
    grad[~keep] = 0
    loss = F(term.reshape(B * K, hw)[keep].astype(np.float64).sum() * (1.0 / n))
    return loss, grad.reshape(B, K, h, w)


MSE_SHAPES = ((1, 1, 2, 2), (2, 17, 8, 8), (1, 3, 2, 6), (2, 5, 36, 30), (61, 17, 4, 4), (129, 16, 2, 2), (3, 17, 64, 64))
MSE_MASKS = ("ones", "zeros", "binary", "fractional")
MSE_SCALES = (1e-3, 1.0, 1e4)
MSE_LAYOUTS = ("contiguous", "front", "back")  # the whole tensor; channels [:K] / [K:] of a [B,2K,h,w] tensor


def mse_cases():
    """-> names "BxKxhxw/mask/scale/layout": every shape with every mask and scale, the three layouts in turn (each shape meets each), and
    one case with pred == target"""
    out = []
    for si, shape in enumerate(MSE_SHAPES):
        for mi, mask in enumerate(MSE_MASKS):
            for ci, scale in enumerate(MSE_SCALES):
                out.append((shape, mask, scale, MSE_LAYOUTS[(si + mi + ci) % 3], False))
    out.append(((2, 17, 8, 8), "binary", 1.0, "front", True))
    return out


def mse_name(case):
    shape, mask, scale, layout, equal = case
    return "x".join(map(str, shape)) + f"/{mask}/{scale:g}/{layout}" + ("/equal" if equal else "")


@functools.lru_cache(maxsize=None)
def mse_operands(case):
    """-> fp32 pred, target, mask (read-only).  Targets are non-negative like heatmaps, the prediction is off by a tenth of the scale."""
    shape, mask, scale, _, equal = case
    B, K, h, w = shape
    rng = np.random.default_rng(zlib.crc32(repr((shape, mask, scale)).encode()))
    target = (rng.random(shape) * scale).astype(F)
    pred = target.copy() if equal else (target + rng.standard_normal(shape) * 0.1 * scale).astype(F)
    if mask == "ones":
        m = np.ones((B, h, w), F)
    elif mask == "zeros":
        m = np.zeros((B, h, w), F)
    elif mask == "binary":
        m = (rng.random((B, h, w)) < 0.6).astype(F)
        m[0].reshape(-1)[0], m[-1].reshape(-1)[-1] = 1, 0  # never constant, even on a 2x2 map
    else:
        m = rng.random((B, h, w)).astype(F)
    for a in (pred, target, m):
        a.setflags(write=False)
    return pred, target, m


@functools.lru_cache(maxsize=None)
def mse_expected(case):
    """-> (loss, grad), (allowed loss, allowed grad): computed once per case"""
    ops = mse_operands(case)
    return mse_reference(*ops), mse_budget(*ops)


# ==================================================================================================================== grouping loss
GROUPING_DEFECTS = ("mean_over_K", "pull_over_listed", "push_n2", "no_minus_n", "push_one_pair", "xy_swapped", "overwrite_shared",
                    "no_div_B", "read_padding")


def grouping_reference(tags, packed, counts, push_scale=1.0, pull_scale=1.0):
    """The grouping loss in fp64, vectorised over the people of an image, with the bookkeeping of the budgets -> namespace: push, pull
    (python floats), grad = push_scale d push / d tags + pull_scale d pull / d tags (fp64), allowed_push, allowed_pull, allowed_grad (the
    budgets, per element), hits (contributions per pixel) and sumabs (the sum of their magnitudes)"""
    T = np.asarray(tags, dtype=np.float64)
    B, K, h, w = T.shape
    P = packed.shape[1]
    push_b, pull_b = np.zeros(B), np.zeros(B)
    e_push_b, e_pull_b = np.zeros(B), np.zeros(B)
    grad = np.zeros((B, K * h * w))
    hits = np.zeros((B, K * h * w), np.int64)
    sumabs, e64 = np.zeros((B, K * h * w)), np.zeros((B, K * h * w))
    for b in range(B):
        npb = min(int(counts[b]), P)
        if npb == 0:
            continue
        J = packed[b, :npb].astype(np.int64)
        vis = J[..., 2] > 0
        x, y = np.where(vis, J[..., 0], 0), np.where(vis, J[..., 1], 0)
        kk = np.broadcast_to(np.arange(K), vis.shape)
        t = np.where(vis, T[b][kk, y, x], 0.0)
        cnt = vis.sum(1)
        has = cnt > 0
        nobj = int(has.sum())
        if nobj == 0:
            continue
        n = np.maximum(cnt, 1)
        m = t.sum(1) / n
        d = np.where(vis, t - m[:, None], 0.0)
        pull_b[b] = ((d * d).sum(1) / n)[has].sum() / nobj
        e_m = (n + 1) * V * np.abs(t).sum(1) / n
        e_d = e_m[:, None] + V * np.abs(d)
        e_pull_b[b] = ((2 * np.abs(d) * e_d + (n[:, None] + 3) * V * d * d).sum(1) / n)[has].sum() / nobj
        dref, e_dref = np.zeros(npb), np.zeros(npb)
        if nobj > 1:
            c = 0.5 / ((nobj - 1.0) * nobj)
            r = m[has]
            D = r[:, None] - r[None, :]
            e = np.exp(-D * D)
            push_b[b] = (e.sum() - nobj) * c
            dref[has] = (-4.0 * D * e).sum(1) * c
            e_D = e_m[has][:, None] + e_m[has][None, :] + V * np.abs(D)
            rel_e = 2 * np.abs(D) * e_D + V * D * D + EXP_REL
            off = ~np.eye(nobj, dtype=bool)
            e_push_b[b] = c * ((e * rel_e)[off].sum() + (P + 10) * V * e.sum())
            e_dref[has] = c * ((4 * (e_D * e + np.abs(D) * e * rel_e)).sum(1) + (P + 10) * V * (4 * np.abs(D) * e).sum(1))
        ps, ls = push_scale / B, pull_scale / B / nobj
        contrib = (ps * dref / n)[:, None] + ls * 2.0 * d / n[:, None]
        e_c = (abs(ps) * e_dref / n)[:, None] + abs(ls) * 2.0 / n[:, None] * (e_m[:, None] + 6 * V * np.abs(d))
        idx = (kk * h * w + y * w + x)[vis]
        cv = contrib[vis]
        np.add.at(grad[b], idx, cv)
        np.add.at(hits[b], idx, 1)
        np.add.at(sumabs[b], idx, np.abs(cv))
        np.add.at(e64[b], idx, e_c[vis])
    push, pull = push_b.sum() / B, pull_b.sum() / B
    shape = (B, K, h, w)
    a_push = U * abs(push) + 2 * (e_push_b.sum() / B + (B + 3) * V * abs(push)) + SUB
    a_pull = U * abs(pull) + 2 * (e_pull_b.sum() / B + (P + B + 6) * V * abs(pull)) + SUB
    order = np.where(hits == 2, U * np.abs(grad) + U * U * sumabs, np.where(hits >= 3, (hits - 1) * U * sumabs, 0.0))
    a_grad = U * sumabs + 2 * e64 + hits * SUB + order
    return SimpleNamespace(push=push, pull=pull, grad=grad.reshape(shape), allowed_push=a_push, allowed_pull=a_pull,
                           allowed_grad=a_grad.reshape(shape), hits=hits.reshape(shape), sumabs=sumabs.reshape(shape))


def grouping_model(tags, packed, counts, push_scale=1.0, pull_scale=1.0, defect=None):
    """ae_grouping_kernel + ae_finalize_kernel restated loop by loop, sharing no code with the reference above: person by person and joint
    by joint in the kernel's order, python floats (double) for the sums, every contribution rounded once to fp32 and added in fp32 onto the
    map -> push, pull (fp32), gradient (fp32) as a correct kernel computes them, or one with `defect` planted.  (The double sums run in
    index order here and as a shuffle tree in the kernel: the difference is what E_push / E_pull / E_i of the budget are for; the model
    tests the fp32 part of the budget and the defects, the MI355X run and oracle/loss.py test the fp64 part.)"""
    T = np.asarray(tags, dtype=F)
    B, K, h, w = T.shape
    P = packed.shape[1]
    grad = np.zeros((B, K, h, w), F)
    per_push, per_pull = [0.0] * B, [0.0] * B
    div_b = 1 if defect == "no_div_B" else B
    for b in range(B):
        listed = P if defect == "read_padding" else min(int(counts[b]), P)
        people = []  # (joints [(k, y, x)], their tags, divisor, mean)
        pull_acc = 0.0
        for p in range(listed):
            js = [(k, int(j[1]), int(j[0])) for k, j in enumerate(packed[b, p]) if j[2] > 0]
            if defect == "xy_swapped":
                js = [(k, x, y) for k, y, x in js]
            t = [float(T[b, k, y, x]) for k, y, x in js]
            if not t:
                continue
            n = K if defect == "mean_over_K" else len(t)
            m = sum(t) / n
            pull_acc += sum((tk - m) * (tk - m) for tk in t) / n
            people.append((js, t, n, m))
        nobj = len(people)
        if nobj == 0:
            continue
        pull_div = listed if defect == "pull_over_listed" else nobj
        per_pull[b] = pull_acc / pull_div
        dref = [0.0] * nobj
        if nobj > 1:
            c = 0.5 / (nobj * nobj) if defect == "push_n2" else 0.5 / ((nobj - 1.0) * nobj)
            means = np.array([q[3] for q in people])
            acc = 0.0
            for a in range(nobj):
                d = means[a] - means
                e = np.exp(-d * d)
                acc += float(e.sum())
                dref[a] = float(((-2.0 if defect == "push_one_pair" else -4.0) * d * e).sum()) * c
            per_push[b] = (acc - (0 if defect == "no_minus_n" else nobj)) * c
        ps, ls = push_scale / div_b, pull_scale / div_b / pull_div
        for (js, t, n, m), g in zip(people, dref):
            gp = ps * g / n
            for (k, y, x), tk in zip(js, t):
                c32 = F(gp + ls * 2.0 * (tk - m) / n)
                grad[b, k, y, x] = c32 if defect == "overwrite_shared" else F(grad[b, k, y, x] + c32)
    return F(sum(per_push) / div_b), F(sum(per_pull) / div_b), grad


def autograd_tags_budget(gpush, gpull, a, b):
    """allowed |error| of fl(fl(gpush a) + fl(gpull b)) against gpush.grad * a + gpull.grad * b, a and b the exact incoming factors (the
    1e-3 of AEKeypointsLoss included) -> reference, allowed"""
    ref = gpush.grad * a + gpull.grad * b
    return ref, abs(a) * gpush.allowed_grad + abs(b) * gpull.allowed_grad + 4 * U * (np.abs(gpush.grad * a) + np.abs(gpull.grad * b))


# ---- the grouping lattice.  A case = tags fp32 [B,K,h,w] (a channel slice where stated), packed int32 [B,P,K,3] (x, y, vis) with P one
# more than the longest list, counts int32 [B].  Visible joints carry vis 1 or 2, invisible ones 0 or -1 and a random in-range position;
# the padding holds VISIBLE people at in-range positions: garbage that a correct kernel never reads and a wrong one cannot fault on.
def _people(rng, K, h, w, n, vis_prob, xmax=None, ymax=None):
    J = np.zeros((n, K, 3), np.int32)
    J[..., 0] = rng.integers(0, xmax or w, (n, K))
    J[..., 1] = rng.integers(0, ymax or h, (n, K))
    visible = rng.random((n, K)) < vis_prob
    J[..., 2] = np.where(visible, rng.integers(1, 3, (n, K)), rng.integers(-1, 1, (n, K)))
    return J


def _make(name, B, K, h, w, counts, vis_prob=0.8, tags="normal", tag_scale=1.0, sliced=False, edit=None, pad=1, swap_safe=False):
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    counts = np.asarray(counts, np.int32)
    assert len(counts) == B
    P = max(1, int(counts.max())) + pad
    packed = np.zeros((B, P, K, 3), np.int32)
    for b in range(B):
        packed[b] = _people(rng, K, h, w, P, 1.0)  # the padding: visible garbage
        if swap_safe:  # positions in range both ways and off the diagonal
            lim = min(h, w)
            J = _people(rng, K, h, w, int(counts[b]), vis_prob, lim, lim)
            J[..., 1] = np.where(J[..., 1] == J[..., 0], (J[..., 0] + 1) % lim, J[..., 1])
            packed[b, :counts[b]] = J
        else:
            packed[b, :counts[b]] = _people(rng, K, h, w, int(counts[b]), vis_prob)
    wide = (rng.standard_normal((B, 2 * K if sliced else K, h, w)) * tag_scale).astype(F)
    T = wide[:, K:] if sliced else wide
    if edit:
        edit(packed, counts, T, rng)
    if tags == "identical":
        T[...] = F(0.7)
    elif tags == "apart40":  # person p of an image sits at 40 p (+ noise): exp(-1600) is 0 in double
        for b in range(B):
            for p in range(int(counts[b])):
                for k in range(K):
                    if packed[b, p, k, 2] > 0:
                        T[b, k, packed[b, p, k, 1], packed[b, p, k, 0]] = F(40.0 * p + 0.1 * rng.standard_normal())
    for a in (T, wide, packed, counts):
        a.setflags(write=False)
    return SimpleNamespace(name=name, tags=T, wide=wide, sliced=sliced, packed=packed, counts=counts, B=B, K=K, h=h, w=w, P=P,
                           swap_safe=swap_safe)


def _edit_hole(packed, counts, T, rng):  # the middle one of three has no visible joint
    packed[0, 1, :, 2] = 0
    packed[0, 0, 0, 2] = packed[0, 2, 0, 2] = 1


def _edit_nobody(packed, counts, T, rng):
    packed[0, :counts[0], :, 2] = rng.integers(-1, 1, (counts[0], packed.shape[2]))


def _edit_one_of_three(packed, counts, T, rng):
    packed[0, 0, :, 2] = 0
    packed[0, 2, :, 2] = -1
    packed[0, 1, :3, 2] = 1


def _edit_single_joint(packed, counts, T, rng):
    K = packed.shape[2]
    for p in range(counts[0]):
        packed[0, p, :, 2] = 0
        packed[0, p, p % K, 2] = 2


def _distinct(packed, counts, T, rng):  # no two people of an image on one pixel
    h, w = T.shape[2:]
    for b in range(len(counts)):
        for k in range(packed.shape[2]):
            pix = rng.permutation(h * w)[:counts[b]]
            packed[b, :counts[b], k, 0], packed[b, :counts[b], k, 1] = pix % w, pix // w


def _edit_shared(n):
    def edit(packed, counts, T, rng):  # the first n people put joint 2 on pixel (x 7, y 3), everything else stays apart
        _distinct(packed, counts, T, rng)
        packed[0, :n, 2] = (7, 3, 1)
    return edit


def _edit_corners(packed, counts, T, rng):
    h, w = T.shape[2:]
    _distinct(packed, counts, T, rng)
    for p, (x, y) in enumerate(((0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1))):
        packed[0, p, :, :2] = (x, y)
        packed[0, p, p, 2] = packed[0, p, 4, 2] = 1


@functools.lru_cache(maxsize=None)
def grouping_cases():
    """-> {name: case}, built once"""
    rag = np.random.default_rng(5).integers(0, 4, 513)
    cases = [
        _make("ragged_0_to_33", 7, 17, 32, 32, (0, 1, 2, 4, 5, 9, 33)),
        _make("K1_four_people", 1, 1, 4, 4, (4,), vis_prob=1.0),
        _make("K5_five_people", 3, 5, 6, 20, (5, 2, 4)),
        _make("K17_tall_map", 3, 17, 20, 6, (9, 0, 1)),
        _make("K64", 1, 64, 32, 32, (5,)),
        _make("K65", 3, 65, 6, 20, (4, 5, 2)),
        _make("K130", 1, 130, 20, 6, (9,)),
        _make("P257_P300", 2, 2, 32, 32, (257, 300), vis_prob=0.9, edit=_distinct, pad=0),
        _make("B513", 513, 2, 4, 4, rag, vis_prob=0.9),
        _make("hole_between_two", 1, 5, 6, 20, (3,), edit=_edit_hole),
        _make("nobody_visible", 1, 5, 6, 20, (3,), edit=_edit_nobody),
        _make("one_of_three_visible", 1, 5, 6, 20, (3,), edit=_edit_one_of_three),
        _make("single_visible_joint", 1, 5, 6, 20, (4,), edit=_edit_single_joint),
        _make("two_on_one_pixel", 1, 5, 6, 20, (3,), vis_prob=1.0, edit=_edit_shared(2)),
        _make("five_on_one_pixel", 1, 5, 6, 20, (5,), vis_prob=1.0, edit=_edit_shared(5)),
        _make("four_corners", 1, 5, 6, 20, (4,), edit=_edit_corners),
        _make("identical_tags", 2, 5, 6, 20, (3, 2), tags="identical"),
        _make("tags_40_apart", 2, 5, 6, 20, (3, 4), edit=_distinct, tags="apart40"),
        _make("tags_1e4", 2, 5, 6, 20, (3, 4), tag_scale=1e4),
        _make("tags_channel_slice", 2, 5, 20, 6, (3, 4), sliced=True),
        _make("swap_safe_wide_map", 2, 5, 6, 20, (4, 3), vis_prob=1.0, swap_safe=True),
    ]
    return {c.name: c for c in cases}


SCALES = ((1.0, 0.0), (0.0, 1.0), (0.25, 3.0))  # d push, d pull, and both in one launch


@functools.lru_cache(maxsize=None)
def grouping_expected(name, push_scale, pull_scale):
    c = grouping_cases()[name]
    return grouping_reference(c.tags, c.packed, c.counts, push_scale, pull_scale)


def joints_lists(case):
    """the case as AEGroupingLoss takes it: a list over images of int32 [P_b,K,3]"""
    return [case.packed[b, :case.counts[b]].copy() for b in range(case.B)]


def pad_to(case, P):
    """the case's joints padded to P people per image, the padding again visible in-range garbage -> packed int32 [B,P,K,3]"""
    rng = np.random.default_rng(P)
    packed = np.stack([_people(rng, case.K, case.h, case.w, P, 1.0) for _ in range(case.B)])
    packed[:, :case.P] = case.packed
    return packed
