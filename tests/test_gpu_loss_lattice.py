"""-m gpu: the training objective (csrc/loss_kernels.hip) through the C-ABI and through keypoints/loss.py, element by element against the
fp64 references and the derived budgets of tests/loss_budget.py.

1. C-ABI: hh_loss_heatmaps and hh_loss_ae_grouping over the lattices; every call twice with identical bits (except gradient pixels that
   receive three or more atomic contributions, whose order is free: there only the budget holds), grad = NULL with the same loss bits,
   both scales in one launch, the ADD into a pre-filled map, the scratch and every neighbouring buffer left alone, P = 2048.
2. The modules: HeatmapsLoss / AEGroupingLoss / AEKeypointsLoss through autograd with GradScaler's factor, fp16 / bf16 predictions,
   bool masks, host targets, channels-last and misaligned views, DeviceJoints.
3. Non-finite predictions, and the refusals.
A visible joint handed to the C-ABI is always inside the map (the header leaves that check to the caller); nothing here relies on what
happens otherwise.
"""
import importlib
import time

import numpy as np
import pytest
import torch

import loss_budget as lb
from conftest import PKG

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 12345.0
WORST = {}
T0 = time.time()
MSE = {lb.mse_name(c): c for c in lb.mse_cases()}


@pytest.fixture(scope="module")
def lossmod():
    return importlib.import_module(PKG + ".keypoints.loss")


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg._lib.load()


def _note(key, got, ref, allowed):
    r = lb.worst(got, ref, allowed)
    WORST[key] = max(WORST.get(key, 0.0), r)
    return r


def _dev(a, dtype=None):
    return torch.tensor(np.ascontiguousarray(a), device=DEV, dtype=dtype)  # (always a copy: the lattice's arrays stay read-only)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _mse_case(prefix):
    (name,) = [n for n in MSE if n.rsplit("/", 1)[0] == prefix]
    return MSE[name]


def _place(a, layout):
    """fp32 [B,K,h,w] on the device -> (the tensor in `layout`, the allocation that holds it); a slice's other half holds sentinels"""
    t = _dev(a)
    if layout == "contiguous":
        return t, t
    B, K, h, w = a.shape
    wide = torch.full((B, 2 * K, h, w), SENTINEL, device=DEV)
    view = wide[:, :K] if layout == "front" else wide[:, K:]
    view.copy_(t)
    return view, wide


def _other_half_intact(view, wide, layout):
    if layout == "contiguous":
        return True
    K = view.shape[1]
    other = wide[:, K:] if layout == "front" else wide[:, :K]
    return bool((other == SENTINEL).all())


def _run_mse(pkg, lib, case, with_grad=True, pred=None, mask=None):
    """hh_loss_heatmaps on one lattice case -> loss (fp32 scalar), gradient (fp32 numpy or None); asserts that nothing around the outputs moved"""
    p0, t0, m0 = lb.mse_operands(case)
    p0, m0 = (p0 if pred is None else pred), (m0 if mask is None else mask)
    layout = case[3]
    B, K, h, w = p0.shape
    p, pwide = _place(p0, layout)
    t, m = _dev(t0), _dev(m0)
    loss = torch.full((3,), SENTINEL, device=DEV)
    scratch = torch.full((1024 + 2,), SENTINEL, device=DEV, dtype=torch.float64)
    g, gwide = _place(np.full(p0.shape, SENTINEL, np.float32), layout) if with_grad else (None, None)
    assert p.data_ptr() % 16 == 0 and (g is None or g.data_ptr() % 16 == 0)
    pkg._lib.check(lib.hh_loss_heatmaps(p.data_ptr(), p.stride(0), t.data_ptr(), m.data_ptr(), B, K, h, w, loss[1:].data_ptr(),
                                        g.data_ptr() if with_grad else None, g.stride(0) if with_grad else 0, scratch.data_ptr(),
                                        torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert loss[0].item() == SENTINEL and loss[2].item() == SENTINEL and bool((scratch[1024:] == SENTINEL).all())
    assert _other_half_intact(p, pwide, layout) and np.array_equal(_bits(p.cpu().numpy()), _bits(p0))  # the inputs are only read
    if with_grad:
        assert _other_half_intact(g, gwide, layout)
    return loss[1].cpu().numpy(), (g.cpu().numpy() if with_grad else None)


# ================================================================================================================= 1. C-ABI, masked MSE
@pytest.mark.parametrize("shape", lb.MSE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_mse_lattice_through_the_c_abi(pkg, lib, shape):
    for name, case in MSE.items():
        if case[0] != shape:
            continue
        (loss, grad), (a_loss, a_grad) = lb.mse_expected(case)
        got_loss, got_grad = _run_mse(pkg, lib, case)
        r = _note("mse loss", got_loss, loss, a_loss), _note("mse grad", got_grad, grad, a_grad)
        print(f"{name}: worst error / budget  loss {r[0]:.3f}  gradient {r[1]:.3f}")
        assert all(v < 1 for v in r), (name, r)
        if case[1] == "zeros" or case[4]:
            assert got_loss == 0 and not got_grad.any(), name
        again_loss, again_grad = _run_mse(pkg, lib, case)
        assert _bits(again_loss) == _bits(got_loss) and np.array_equal(_bits(again_grad), _bits(got_grad)), name
        alone, _ = _run_mse(pkg, lib, case, with_grad=False)
        assert _bits(alone) == _bits(got_loss), name


# =============================================================================================================== 1. C-ABI, grouping loss
def _run_grouping(pkg, lib, c, push_scale, pull_scale, with_grad=True, prefill=0.0, packed=None):
    """hh_loss_ae_grouping -> push, pull (fp32 scalars), the map the gradient was added to (numpy or None).  The scratch is exactly
    max(1024, 2 B) doubles, the gradient of a sliced case lands in a channel slice."""
    packed = c.packed if packed is None else packed
    B, P, K, h, w = c.B, packed.shape[1], c.K, c.h, c.w
    if c.sliced:
        twide = _dev(c.wide)
        t = twide[:, K:]
        gwide = torch.full((B, 2 * K, h, w), SENTINEL, device=DEV)
        g = gwide[:, K:]
        g.fill_(prefill)
    else:
        t = twide = _dev(c.tags)
        g = gwide = torch.full((B, K, h, w), prefill, device=DEV)
    pk, cn = _dev(packed), _dev(c.counts)
    out = torch.full((4,), SENTINEL, device=DEV)
    n = max(1024, 2 * B)
    scratch = torch.full((n + 2,), SENTINEL, device=DEV, dtype=torch.float64)
    pkg._lib.check(lib.hh_loss_ae_grouping(t.data_ptr(), t.stride(0), pk.data_ptr(), cn.data_ptr(), B, P, K, h, w, out[1:].data_ptr(),
                                           g.data_ptr() if with_grad else None, g.stride(0) if with_grad else 0, push_scale, pull_scale,
                                           scratch.data_ptr(), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert out[0].item() == SENTINEL and out[3].item() == SENTINEL and bool((scratch[n:] == SENTINEL).all())
    assert np.array_equal(_bits(twide.cpu().numpy()), _bits(c.wide)) and (not c.sliced or bool((gwide[:, :K] == SENTINEL).all()))
    push, pull = out[1:3].cpu().numpy()
    return push, pull, (g.cpu().numpy() if with_grad else None)


def _check_grouping(pkg, lib, c, ref, ps, ls, what, packed=None):
    push, pull, grad = _run_grouping(pkg, lib, c, ps, ls, packed=packed)
    r = (_note("push", push, ref.push, ref.allowed_push), _note("pull", pull, ref.pull, ref.allowed_pull),
         _note(what, grad, ref.grad, ref.allowed_grad))
    print(f"{c.name} scales ({ps:g}, {ls:g}): worst error / budget  push {r[0]:.3f}  pull {r[1]:.3f}  gradient {r[2]:.3f}")
    assert all(v < 1 for v in r), (c.name, ps, ls, r)
    assert not grad[ref.hits == 0].any(), c.name
    return push, pull, grad


@pytest.mark.parametrize("name", list(lb.grouping_cases()))
def test_grouping_lattice_through_the_c_abi(pkg, lib, name):
    c = lb.grouping_cases()[name]
    for (ps, ls), what in zip(lb.SCALES, ("d push", "d pull", "0.25 d push + 3 d pull")):
        ref = lb.grouping_expected(name, ps, ls)
        push, pull, grad = _check_grouping(pkg, lib, c, ref, ps, ls, what)
        push2, pull2, grad2 = _run_grouping(pkg, lib, c, ps, ls)
        assert _bits(push2) == _bits(push) and _bits(pull2) == _bits(pull), name
        # THE exception to "twice, identical bits": a pixel that three or more people hit sums its contributions in the order the atomics
        # arrive.  Two contributions commute, so every other pixel must repeat bit for bit; the budget above holds for all of them.
        fixed = ref.hits <= 2
        assert np.array_equal(_bits(grad2)[fixed], _bits(grad)[fixed]), name
        push3, pull3, _ = _run_grouping(pkg, lib, c, ps, ls, with_grad=False)
        assert _bits(push3) == _bits(push) and _bits(pull3) == _bits(pull), name
        # the special cases whose reference is an exact zero
        if name == "nobody_visible":
            assert push == 0 and pull == 0 and not grad.any()
        if name == "one_of_three_visible":
            assert push == 0 and (ls != 0 or not grad.any())
        if name == "single_visible_joint":
            assert pull == 0 and (ps != 0 or not grad.any())
    # the kernel ADDS to the map (include/hhrnet.h): every pixel it does not touch keeps the 1.5 it held, the others gain the gradient
    ps, ls = lb.SCALES[2]
    ref = lb.grouping_expected(name, ps, ls)
    _, _, filled = _run_grouping(pkg, lib, c, ps, ls, prefill=1.5)
    assert (filled[ref.hits == 0] == 1.5).all(), name
    allowed = ref.allowed_grad + ref.hits * lb.U * (1.5 + ref.sumabs)  # one more rounding per addition, now on values up to 1.5 + sum|c|
    assert _note("added onto a filled map", filled, 1.5 + ref.grad, allowed) < 1, name


def test_the_cap_of_2048_people(pkg, lib):
    """P = 2048 is the largest LDS request (40 992 bytes); three of the 2048 listed people are valid"""
    c = lb.grouping_cases()["two_on_one_pixel"]
    assert list(c.counts) == [3]
    packed = lb.pad_to(c, 2048)
    ps, ls = lb.SCALES[2]
    ref = lb.grouping_reference(c.tags, packed, c.counts, ps, ls)
    _check_grouping(pkg, lib, c, ref, ps, ls, "0.25 d push + 3 d pull", packed=packed)


# ======================================================================================================================== 2. the modules
def _t(a, dtype="float32"):
    return _dev(a).to(getattr(torch, dtype))


def _f32(t):
    return t.detach().float().cpu().numpy()


@pytest.mark.parametrize("dtype", ["float32", "float16", "bfloat16"])
def test_heatmaps_loss_with_the_scalers_factor(lossmod, dtype):
    """(loss * 65536).backward() on a channel slice, the form the net emits.  In fp16 a gradient of 1e-8 is below half the smallest
    subnormal: it must come back non-zero because the factor is applied before the cast."""
    case = _mse_case("3x17x64x64/binary/1")
    pred, target, mask = lb.mse_operands(case)
    K = pred.shape[1]
    wide = torch.cat([_t(pred, dtype), _t(pred, dtype)], 1).requires_grad_()
    seen = _f32(wide[:, :K])  # what the kernel reads: the narrow values, widened exactly
    (loss, grad), (a_loss, a_grad) = lb.mse_reference(seen, target, mask), lb.mse_budget(seen, target, mask)
    out = lossmod.HeatmapsLoss()(wide[:, :K], _dev(target), _dev(mask))
    (out * 65536.0).backward()
    assert out.dtype == torch.float32 and wide.grad.dtype == getattr(torch, dtype) and not wide.grad[:, K:].any()
    got = _f32(wide.grad[:, :K])
    want = 65536.0 * grad
    allowed = 65536.0 * (a_grad + lb.U * np.abs(grad)) + (lb.half_ulp(want, dtype) if dtype != "float32" else 0.0)
    r = _note("mse loss", out.item(), loss, a_loss), _note(f"mse grad x 65536 -> {dtype}", got, want, allowed)
    print(f"HeatmapsLoss {dtype}: worst error / budget  loss {r[0]:.3f}  gradient {r[1]:.3f}")
    assert all(v < 1 for v in r), r
    tiny = (np.abs(grad) > 5e-9) & (np.abs(grad) < 2e-8)
    assert tiny.sum() > 100 and (got[tiny] != 0).all()


def test_heatmaps_loss_input_forms_give_the_same_bits(pkg, lib, lossmod):
    """a bool mask, targets on the host, a channels-last prediction (copied) and views that start at an odd element of a larger
    allocation (copied: the kernel moves float4) all give the bits of the plain call, which gives the bits of the C-ABI"""
    case = _mse_case("2x17x8x8/binary/1")
    pred, target, mask = lb.mse_operands(case)
    base_loss, base_grad = _run_mse(pkg, lib, case)

    def run(p, t, m):
        p = p.requires_grad_()
        out = lossmod.HeatmapsLoss()(p, t, m)
        out.backward()
        assert p.grad.shape == p.shape
        return _bits(out.detach().cpu().numpy()), _bits(p.grad.cpu().numpy())

    def odd(a):  # a contiguous view one element into a larger allocation, wholly inside it
        big = torch.full((a.size + 8,), SENTINEL, device=DEV)
        v = big[1:1 + a.size].view(a.shape)
        v.copy_(_dev(a))
        assert v.data_ptr() % 16 == 4 and v.is_contiguous()
        return v, big

    forms = {
        "plain": (_dev(pred), _dev(target), _dev(mask)),
        "bool mask": (_dev(pred), _dev(target), _dev(mask) > 0),
        "host targets": (_dev(pred), torch.tensor(target), torch.tensor(mask)),
        "channels last": (_dev(pred).to(memory_format=torch.channels_last), _dev(target), _dev(mask)),
    }
    (po, pbig), (to, tbig), (mo, mbig) = odd(pred), odd(target), odd(mask)
    forms["odd views"] = (po.detach(), to, mo)
    for what, (p, t, m) in forms.items():
        loss_bits, grad_bits = run(p, t, m)
        assert loss_bits == _bits(base_loss) and np.array_equal(grad_bits, _bits(base_grad)), what
    for big in (pbig, tbig, mbig):
        assert big[0].item() == SENTINEL and bool((big[-7:] == SENTINEL).all())
    # the C-ABI itself refuses each misaligned pointer before the launch: the outputs keep their sentinels
    loss = torch.full((1,), SENTINEL, device=DEV)
    g = torch.full(pred.shape, SENTINEL, device=DEV)
    gbig = torch.full((pred.size + 8,), SENTINEL, device=DEV)
    scratch = torch.zeros(1024, device=DEV, dtype=torch.float64)
    P, T, M = _dev(pred), _dev(target), _dev(mask)
    B, K, h, w = pred.shape
    for what, args in (("pred", (po, T, M, g)), ("target", (P, to, M, g)), ("mask", (P, T, mo, g)), ("grad", (P, T, M, gbig[1:]))):
        rc = lib.hh_loss_heatmaps(args[0].data_ptr(), K * h * w, args[1].data_ptr(), args[2].data_ptr(), B, K, h, w, loss.data_ptr(),
                                  args[3].data_ptr(), K * h * w, scratch.data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert rc != 0 and "16-byte aligned" in lib.hh_last_error().decode(), what
    torch.cuda.synchronize()
    assert loss.item() == SENTINEL and bool((g == SENTINEL).all()) and bool((gbig == SENTINEL).all())


def test_device_joints_and_host_lists_give_the_same_bits(lossmod):
    c = lb.grouping_cases()["K5_five_people"]
    joints = lb.joints_lists(c)
    fn = lossmod.AEGroupingLoss()
    outs = []
    for j in (joints, lossmod.upload_joints(joints, c.K, c.h, c.w, DEV),
              lossmod.DeviceJoints(_dev(c.packed), _dev(c.counts), (c.K, c.h, c.w))):  # the last with garbage in its padding
        t = _dev(c.tags).requires_grad_()
        push, pull = fn(t, j)
        (push + pull).backward()
        outs.append((_bits(np.float32(push.item())), _bits(np.float32(pull.item())), _bits(t.grad.cpu().numpy())))
    for o in outs[1:]:
        assert all(np.array_equal(a, b) for a, b in zip(o, outs[0]))
    ref = lb.grouping_expected(c.name, 1.0, 1.0)
    push, pull = fn(_dev(c.tags), joints)
    assert abs(push.item() - ref.push) < ref.allowed_push and abs(pull.item() - ref.pull) < ref.allowed_pull


@pytest.mark.parametrize("dtype", ["float32", "float16", "bfloat16"])
def test_ae_keypoints_loss_through_autograd(lossmod, dtype):
    """AEKeypointsLoss.calculate_loss on the net's layout (stage-0 heatmaps and tags are channel slices of one tensor), the sum of the four
    losses times 65536 backwards: every loss and every gradient element against the references"""
    c = lb.grouping_cases()["K5_five_people"]
    B, K, h, w = c.B, c.K, c.h, c.w
    stage = [((B, K, h, w), "binary", 1.0, "front", False), ((B, K, 2 * h, 2 * w), "fractional", 1.0, "contiguous", False)]
    ops = [lb.mse_operands(s) for s in stage]
    init = torch.cat([_t(ops[0][0], dtype), _t(c.tags, dtype)], 1).requires_grad_()
    dec = _t(ops[1][0], dtype).requires_grad_()
    seen = [_f32(init[:, :K]), _f32(dec)]
    tags_seen = _f32(init[:, K:])
    hl, push, pull = lossmod.AEKeypointsLoss().calculate_loss([init[:, :K], dec], init[:, K:], [_dev(o[1]) for o in ops], [_dev(o[2]) for o in ops],
                                                              [lb.joints_lists(c), None])
    ((hl[0] + hl[1] + push[0] + pull[0]) * 65536.0).backward()
    assert init.grad.dtype == dec.grad.dtype == getattr(torch, dtype)
    narrow = (lambda x: lb.half_ulp(x, dtype)) if dtype != "float32" else (lambda x: 0.0)
    worst = {}
    for i, got in enumerate((_f32(init.grad[:, :K]), _f32(dec.grad))):
        (loss, grad), (a_loss, a_grad) = lb.mse_reference(seen[i], *ops[i][1:]), lb.mse_budget(seen[i], *ops[i][1:])
        want = 65536.0 * grad
        worst[f"hm{i}"] = _note("mse loss", hl[i].item(), loss, a_loss)
        worst[f"d hm{i}"] = _note(f"mse grad x 65536 -> {dtype}", got, want, 65536.0 * (a_grad + lb.U * np.abs(grad)) + narrow(want))
    gp = lb.grouping_reference(tags_seen, c.packed, c.counts, 1.0, 0.0)
    gl = lb.grouping_reference(tags_seen, c.packed, c.counts, 0.0, 1.0)
    # the losses: fl(1e-3) and the product, two roundings on top of the kernel's
    worst["push"] = _note("push x 1e-3", push[0].item(), 1e-3 * gp.push, 1e-3 * gp.allowed_push + 2 * lb.U * abs(1e-3 * gp.push))
    worst["pull"] = _note("pull x 1e-3", pull[0].item(), 1e-3 * gl.pull, 1e-3 * gl.allowed_pull + 2 * lb.U * abs(1e-3 * gl.pull))
    want, allowed = lb.autograd_tags_budget(gp, gl, 65.536, 65.536)
    got = _f32(init.grad[:, K:])
    worst["d tags"] = _note(f"tags grad x 65.536 -> {dtype}", got, want, allowed + narrow(want))
    assert not got[gp.hits == 0].any()
    print(f"AEKeypointsLoss {dtype}: worst error / budget " + "  ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert all(v < 1 for v in worst.values()), worst


# ============================================================================================================ 3. non-finite, refusals
@pytest.mark.parametrize("value,masked", [(float("inf"), False), (float("nan"), False), (float("-inf"), True)])
def test_a_non_finite_prediction_shows_where_the_reference_has_it(pkg, lib, value, masked):
    """The fp16 step's overflow detection rests on this: the loss is non-finite as the fp64 reference's is, the gradient at that element
    and at no other (an inf under a zero mask is inf * 0 = NaN in both)."""
    case = _mse_case("2x17x8x8/ones/1")
    pred, target, mask = (a.copy() for a in lb.mse_operands(case))
    where = (1, 7, 2, 5)
    if masked:
        mask[1, 2, 5] = 0
    clean_loss, clean_grad = _run_mse(pkg, lib, case, mask=mask)
    pred[where] = value
    with np.errstate(invalid="ignore", over="ignore"):
        loss, grad = lb.mse_reference(pred, target, mask)
    got_loss, got_grad = _run_mse(pkg, lib, case, pred=pred, mask=mask)
    assert not np.isfinite(loss) and np.isnan(got_loss) == np.isnan(loss) and np.isinf(got_loss) == np.isinf(loss) and got_loss != -loss
    bad = ~np.isfinite(got_grad)
    assert np.array_equal(bad, ~np.isfinite(grad)) and bad.sum() == 1 and bad[where]
    assert np.array_equal(np.isnan(got_grad), np.isnan(grad)) and (got_grad[where] == grad[where] or np.isnan(grad[where]))
    assert np.array_equal(_bits(got_grad)[~bad], _bits(clean_grad)[~bad])  # every other element as in the clean run
    assert np.isfinite(clean_loss)


def test_refusals_arrive_as_exceptions(pkg, lossmod):
    HHError = pkg._lib.HHError
    hm = lossmod.HeatmapsLoss()
    with pytest.raises(HHError, match="multiples of 4"):
        hm(torch.zeros(1, 1, 3, 3, device=DEV), torch.zeros(1, 1, 3, 3, device=DEV), torch.ones(1, 3, 3, device=DEV))
    with pytest.raises(HHError, match="no CPU path"):
        hm(torch.zeros(1, 1, 4, 4), torch.zeros(1, 1, 4, 4), torch.ones(1, 4, 4))
    with pytest.raises(ValueError, match="do not match"):
        hm(torch.zeros(1, 1, 4, 4, device=DEV), torch.zeros(1, 2, 4, 4, device=DEV), torch.ones(1, 4, 4, device=DEV))
    ae = lossmod.AEGroupingLoss()
    tags = torch.zeros(1, 2, 4, 4, device=DEV, requires_grad=True)
    with pytest.raises(HHError, match="2048"):
        ae(tags, [np.ones((2049, 2, 3), np.int32)])
    with pytest.raises(HHError, match="no CPU path"):
        ae(torch.zeros(1, 2, 4, 4), [np.ones((1, 2, 3), np.int32)])
    with pytest.raises(IndexError):
        ae(tags, [np.array([[[4, 0, 1], [0, 0, 1]]], np.int32)])
    with pytest.raises(ValueError, match="entries"):
        ae(tags, [])
    # joints packed for a larger map: their range check does not cover a gather from this one
    big = lossmod.upload_joints([np.array([[[19, 5, 1], [0, 0, 1]]], np.int32)], 2, 6, 20, DEV)
    with pytest.raises(ValueError, match="packed for"):
        ae(tags, big)
    with pytest.raises(ValueError, match="packed for"):
        ae(torch.zeros(1, 2, 20, 6, device=DEV), big)  # the same pixel count, transposed
    push, pull = ae(torch.zeros(1, 2, 6, 20, device=DEV), big)
    assert push.item() == 0 and pull.item() == 0
    assert tags.grad is None


def test_report_worst_ratios(pkg):
    """(runs last in this file) the worst kernel error / budget per output of this process, and the file's wall time"""
    print("worst error / budget: " + "; ".join(f"{k} {v:.3f}" for k, v in sorted(WORST.items())) + f"; wall time {time.time() - T0:.0f} s")
    assert all(v < 1 for v in WORST.values()), WORST
