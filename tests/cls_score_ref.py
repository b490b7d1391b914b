"""The rule of hh_cls_score_batch (include/hhrnet.h) restated in numpy / torch, its fp64 references with per-element error budgets, an
fp32 model of a correct kernel that can plant defects, and the ctypes calls of the library's entry points (a plain module; the unit
roundoffs, EXPF_ULPS, `ranks` and `check` are cls_budget's).

Exact outputs (integers from comparisons of the logits as given): topk_idx, rank, every counter, per_class, conf, flags.
Floating outputs against fp64, with d_j = z_j - m (one fp32 subtraction), e_j = expf(d_j), rho_j = U32 |d_j| + 2 EXPF_ULPS U32 and
rho_bar = sum_j p_j rho_j, the quantities cls_budget derives for dlogits, without its 1 / B and one-hot:
  row loss (double)   rho_bar + (N + 4) U64 (1 + |lse| + |z_t|): xent_refs' per-row term.  It bounds the DOUBLE loss, which the accumulator
                      keeps (loss_sum after one row is that double); the fp32 output row_loss is that double rounded once more, so its
                      budget adds U32 |ref| for the store.
  loss_sum            the sum of the scored rows' budgets + B U64 |sum| (B double additions)
  topk_prob           p (rho_i + rho_bar + 2 U32) for the quotient (as dlogits' p) + U32 p for the one fp32 rounding + 2 TINY32 (an
                      e_j below 2^-126 is subnormal or flushed)
Host expf and device expf differ: there is no bit claim on floating outputs across implementations.
"""
from __future__ import annotations

import numpy as np
import torch

from cls_budget import EXPF_ULPS, TINY32, ranks  # noqa: F401
from train_budget import U32, U64, check

K_MAX = 8
ROW_REGS = 1024  # HH_CLS_ROW_REGS: a longer row is not held in registers
# (B, N, k): the smallest shapes at which the kernel can go wrong
SHAPES = [(1, 1, 1),        # the smallest case
          (1, 5, 5),        # N == k
          (3, 3, 5),        # N < k
          (7, 64, 5),       # one lane stride exactly
          (5, 65, 5),       # one lane stride plus one
          (33, 1000, 5),    # a row count that fills no workgroup evenly
          (4, 1001, 8),     # the largest k
          (3, 1024, 5),     # the longest row held in registers
          (3, 1025, 5)]     # the shortest row read again from memory on every pass
INT_KEYS = ("topk_idx", "rank", "rows", "top1", "topk", "bad_target", "nonfinite", "flags", "per_class", "conf")


def shape_id(s) -> str:
    return "x".join(map(str, s))


def random_case(B: int, N: int, seed: int = 0):
    g = torch.Generator().manual_seed(9000 + 7 * B + N + 1000 * seed)
    z = torch.randn(B, N, generator=g) * 3
    t = torch.randint(0, N, (B,), generator=g)
    t[-1] = N - 1
    return z, t


def content_cases() -> dict:
    """name -> (z fp32 [B,N], t int64 [B])"""
    import cls_budget as cb
    out = {}
    z, t, _ = cb.tie_case()
    out["ties"] = (z, t)
    out["all-equal"] = (torch.full((2, 70), 1.5), torch.tensor([0, 69]))
    z = torch.zeros(2, 130) - 1
    z[0, 0] = z[0, 64] = 2.0       # equal maxima in the same lane
    z[1, 63] = z[1, 64] = 2.0      # equal maxima in neighbouring lanes
    out["equal-maxima"] = (z, torch.tensor([64, 64]))
    z = torch.full((2, 8), -1.0)
    z[0, 2], z[0, 5] = 0.0, -0.0
    z[1, 2], z[1, 5] = -0.0, 0.0
    out["signed-zeros"] = (z, torch.tensor([5, 5]))
    z, t = random_case(4, 70, 1)
    z[0, 3:60] = -np.inf
    z[1, :] = -np.inf
    z[1, 7] = 0.25                 # one finite entry: k - 1 of the top-k are -inf
    z[2, int(t[2])] = -np.inf      # the target itself: loss = +inf
    out["minus-inf"] = (z, t)
    z, t = random_case(5, 66, 2)
    z[1, 65] = np.nan
    z[3, 0] = np.inf
    out["nan-and-inf-rows"] = (z, t)
    out["out-of-range"] = cb.out_of_range_case()
    return out


# ------------------------------------------------------------------------------------------------ the rule
def order(z: torch.Tensor) -> torch.Tensor:
    """[B,N] indices of each row in the rule's order: descending value, ties (-0.0 == +0.0 included) to the lower index.  No NaN."""
    zn = z.numpy().astype(np.float32)
    return torch.from_numpy(np.argsort(-(zn + np.float32(0.0)), axis=1, kind="stable"))  # (+ 0.0 turns -0.0 into +0.0; stable keeps index order)


def nonfinite_rows(z: torch.Tensor) -> torch.Tensor:
    return torch.isnan(z).any(1) | (z == np.inf).any(1) | (z == -np.inf).all(1)


def restate(z: torch.Tensor, t: torch.Tensor | None, k: int, confusion: bool = True) -> dict:
    """The rule on z fp32 [B,N], t int64 [B] or None -> the exact outputs (INT_KEYS), and (fp64 reference, allowed) for topk_prob,
    row_loss (the fp32 output), loss64 (the double loss per row) and loss_sum."""
    B, N = z.shape
    keff = min(k, N)
    nf = nonfinite_rows(z)
    zc = torch.where(nf.view(-1, 1), torch.zeros_like(z), z)  # (placeholders: the rows are masked below)
    idx = torch.full((B, k), -1, dtype=torch.int64)
    idx[:, :keff] = order(zc)[:, :keff]
    idx[nf] = -1
    zd = zc.double()
    m = zd.max(1, keepdim=True).values
    d = zd - m
    s = d.exp().sum(1, keepdim=True)
    lse = m + s.log()
    p = d.exp() / s
    with np.errstate(invalid="ignore"):
        rho = torch.nan_to_num(U32 * d.abs(), posinf=0.0) + 2 * EXPF_ULPS * U32   # (d = -inf: e = 0 exactly, p = 0)
    rho_bar = (p * rho).sum(1, keepdim=True)
    gi = idx.clamp(min=0)
    pk = torch.where(idx >= 0, p.gather(1, gi), torch.zeros(B, k, dtype=torch.float64))
    a_pk = torch.where(idx >= 0, pk * (rho.gather(1, gi) + rho_bar + 2 * U32) + U32 * pk + 2 * TINY32, torch.zeros(B, k, dtype=torch.float64))
    has_t = t is not None
    tt = t if has_t else torch.full((B,), -1, dtype=torch.int64)
    in_range = (tt >= 0) & (tt < N)
    scored = in_range & ~nf
    bad = has_t & ~in_range & ~nf
    tc = tt.clamp(0, N - 1)
    zt = zd.gather(1, tc.view(-1, 1))
    r = ranks(zc, tt, in_range)
    rank = torch.where(scored, r, torch.full_like(r, -1))
    loss = torch.where(scored, (lse - zt).view(-1), torch.zeros(B, dtype=torch.float64))
    with np.errstate(invalid="ignore"):
        a64 = torch.where(scored, (rho_bar + (N + 4) * U64 * (1 + lse.abs() + torch.nan_to_num(zt.abs(), posinf=0.0))).view(-1),
                          torch.zeros(B, dtype=torch.float64))
    out = {"topk_idx": idx.int(), "rank": rank.int(), "topk_prob": (pk, a_pk), "loss64": (loss, a64), "row_loss": (loss, a64 + U32 * torch.nan_to_num(loss.abs(), posinf=0.0)),
           "rows": int(scored.sum()), "top1": int((scored & (r < 1)).sum()), "topk": int((scored & (r < keff)).sum()),
           "bad_target": int(bad.sum()), "nonfinite": int(nf.sum()) if has_t else 0, "scored": scored}
    out["flags"] = (1 if out["bad_target"] else 0) | (2 if out["nonfinite"] else 0)
    pc = torch.zeros(3, N, dtype=torch.int32)
    conf = torch.zeros(N, N, dtype=torch.int32)
    for b in torch.nonzero(scored).view(-1).tolist():
        c = int(tt[b])
        pc[0, c] += 1
        pc[1, c] += int(r[b] < 1)
        pc[2, c] += int(r[b] < keff)
        conf[c, int(idx[b, 0])] += 1
    out["per_class"], out["conf"] = pc, conf if confusion else None
    ls = loss[scored].sum()
    out["loss_sum"] = (ls.reshape(1), (a64[scored].sum() + B * U64 * torch.nan_to_num(ls.abs(), posinf=0.0)).reshape(1))
    return out


# ------------------------------------------------------------------------------------------------ the fp32 model
DEFECTS = ("tie_high", "le_hit", "conf_T", "bad_counted", "nan_scored", "k_unclamped", "fp32_fold")


def model(z: torch.Tensor, t: torch.Tensor, k: int, confusion: bool = True, calls=None, defect: str | None = None) -> dict:
    """The kernel's arithmetic in torch fp32 (the sum of the exponentials, the quotient and the loss in double), row by row over `calls`
    (a split of the B rows; None = one call) -> the outputs under restate's names, floating ones as plain tensors.  defect: one of
    DEFECTS, planted."""
    assert defect is None or defect in DEFECTS
    B, N = z.shape
    keff = min(k, N)
    calls = calls or [B]
    assert sum(calls) == B
    idx = torch.full((B, k), -1, dtype=torch.int32)
    prob = torch.zeros(B, k)
    rank = torch.full((B,), -1, dtype=torch.int32)
    row_loss = torch.zeros(B)
    acc = {"rows": 0, "top1": 0, "topk": 0, "bad_target": 0, "nonfinite": 0, "flags": 0, "per_class": torch.zeros(3, N, dtype=torch.int32),
           "conf": torch.zeros(N, N, dtype=torch.int32), "loss_sum": np.float64(0.0)}
    start = 0
    for n in calls:
        call32 = np.float32(0.0)
        for b in range(start, start + n):
            row = z[b]
            nf = bool(nonfinite_rows(row.view(1, -1))[0])
            if nf and defect != "nan_scored":
                acc["nonfinite"] += 1
                acc["flags"] |= 2
                continue
            if defect == "tie_high":
                o = (N - 1) - order(torch.nan_to_num(row).flip(0).view(1, -1))[0]
            else:
                o = order(torch.nan_to_num(row).view(1, -1))[0]
            m = row.max()
            e = (row - m).exp()
            s = e.double().sum()
            for r in range(k if defect == "k_unclamped" else keff):
                j = int(o[r % N])
                idx[b, r], prob[b, r] = j, (e[j].double() / s).float()
            c = int(t[b])
            if not 0 <= c < N:
                acc["bad_target"] += 1
                acc["flags"] |= 1
                if defect != "bad_counted":
                    continue
                c = min(max(c, 0), N - 1)
            rk = int(ranks(torch.nan_to_num(row).view(1, -1), torch.tensor([c]), torch.tensor([True]))[0])
            if defect == "tie_high":
                rk = int((row > row[c]).sum() + ((row == row[c]) & (torch.arange(N) > c)).sum())
            loss = (m.double() + s.log()) - row[c].double()
            rank[b], row_loss[b] = rk, loss.float()
            hit1, hitk = rk < 1, (rk <= keff if defect == "le_hit" else rk < keff)
            acc["rows"] += 1
            acc["top1"] += hit1
            acc["topk"] += hitk
            acc["per_class"][0, c] += 1
            acc["per_class"][1, c] += int(hit1)
            acc["per_class"][2, c] += int(hitk)
            top0 = int(idx[b, 0])
            if defect == "conf_T":
                acc["conf"][top0, c] += 1
            else:
                acc["conf"][c, top0] += 1
            if defect == "fp32_fold":
                call32 = np.float32(call32 + np.float32(loss))
            else:
                acc["loss_sum"] = acc["loss_sum"] + np.float64(loss)
        start += n
        if defect == "fp32_fold":
            acc["loss_sum"] = np.float64(np.float32(acc["loss_sum"]) + call32)
    acc["loss_sum"] = torch.tensor([acc["loss_sum"]], dtype=torch.float64)
    if not confusion:
        acc["conf"] = None
    return {"topk_idx": idx, "topk_prob": prob, "rank": rank, "row_loss": row_loss, **acc}


def mismatches(got: dict, ref: dict, what: str = "") -> list:
    """-> the names of the outputs of `got` that differ from the exact ones or leave their budget (empty: all inside)"""
    bad = []
    for key in INT_KEYS:
        if key not in got or (got[key] is None and ref[key] is None):
            continue
        g, r = got[key], ref[key]
        same = bool(torch.equal(torch.as_tensor(g).long(), torch.as_tensor(r).long())) if isinstance(r, torch.Tensor) else int(g) == int(r)
        if not same:
            bad.append(key)
    for key in ("topk_prob", "row_loss", "loss_sum"):
        if key in got:
            g, (r, a) = torch.as_tensor(got[key]).double(), ref[key]
            inf = torch.isinf(r)  # (a target at -inf: the loss is +inf on both sides, exactly)
            try:
                assert torch.equal(torch.isinf(g) & (g > 0), inf), f"{what} {key}: +inf at other places"
                check(torch.where(inf, torch.zeros_like(g), g), torch.where(inf, torch.zeros_like(r), r), a, f"{what} {key}", spatial=False)
            except AssertionError:
                bad.append(key)
    return bad


# ------------------------------------------------------------------------------------------------ the library
def _p(a):
    return None if a is None else a.ctypes.data


def host_twin(lib, z: torch.Tensor, t: torch.Tensor | None, k: int, confusion: bool = True, calls=None, with_acc: bool = True) -> dict:
    """hh_cls_score_host over `calls` (a split of the rows; None = one call) on one accumulator -> the outputs under restate's names plus
    "raw": every byte of the accumulator (uint8)."""
    zn = np.ascontiguousarray(z.numpy(), np.float32)
    tn = None if t is None else np.ascontiguousarray(t.numpy(), np.int64)
    B, N = zn.shape
    out = {"topk_idx": np.full((B, k), -7, np.int32), "topk_prob": np.full((B, k), -7, np.float32), "rank": np.full(B, -7, np.int32),
           "row_loss": np.full(B, -7, np.float32)}
    acc = None
    if with_acc:
        acc = np.full(lib.hh_cls_eval_bytes(N, int(confusion)) // 8, -1, np.int64)
        assert lib.hh_cls_eval_reset_host(_p(acc), N, int(confusion)) == 0, lib.hh_last_error()
    b = 0
    for n in calls or [B]:
        rc = lib.hh_cls_score_host(_p(zn[b:]), None if tn is None else _p(tn[b:]), n, N, k, _p(acc), _p(out["topk_idx"][b:]), _p(out["topk_prob"][b:]),
                                   _p(out["rank"][b:]), _p(out["row_loss"][b:]))
        assert rc == 0, lib.hh_last_error()
        b += n
    assert b == B
    out = {key: torch.from_numpy(v) for key, v in out.items()}
    if with_acc:
        out.update(parse_acc(acc.view(np.uint8), N, confusion))
    return out


def parse_acc(raw: np.ndarray, N: int, confusion: bool) -> dict:
    """every byte of an accumulator -> its fields under restate's names, plus "raw" and "scratch" (the bytes behind the tables)"""
    hdr = np.dtype({"names": ["rows", "top1", "topk", "bad_target", "nonfinite", "loss_sum", "flags", "N", "with_confusion", "reserved"],
                    "formats": ["<i8"] * 5 + ["<f8", "<u4", "<i4", "<i4", "<i4"]})
    assert hdr.itemsize == 64
    h = raw[:64].view(hdr)[0]
    out = {key: int(h[key]) for key in ("rows", "top1", "topk", "bad_target", "nonfinite", "flags")}
    assert int(h["N"]) == N and int(h["with_confusion"]) == int(confusion)
    out["loss_sum"] = torch.tensor([float(h["loss_sum"])], dtype=torch.float64)
    out["per_class"] = torch.from_numpy(raw[64:64 + 12 * N].view(np.int32).reshape(3, N).copy())
    end = 64 + 12 * N
    out["conf"] = None
    if confusion:
        out["conf"] = torch.from_numpy(raw[end:end + 4 * N * N].view(np.int32).reshape(N, N).copy())
        end += 4 * N * N
    out["raw"], out["scratch"] = raw.copy(), raw[end:].copy()
    return out
