"""No GPU: the budgets of tests/grad_clip_budget.py are tight enough to catch what can go wrong in csrc/grad_stats.hip, and loose
enough for a correct kernel.  A numpy model of the kernels' own summation order stays inside every budget over the lattice; each
planted defect leaves its budget (or its bit-exact check) on a named case; the exact-arithmetic case reproduces torch bit for bit; the
C-ABI refuses bad arguments on the host; optim.clip_grad_norm_ refuses what it does not cover and hands any other optimizer to torch."""
import importlib

import numpy as np
import pytest
import torch

import grad_clip_budget as gb
from conftest import PKG

F = np.float32
INF = float("inf")


@pytest.fixture(scope="module")
def optim():
    return importlib.import_module(PKG + ".optim")


@pytest.fixture(scope="module")
def lattice():
    """gradients, fp64 reference, budgets and the model's statistics: computed once, read by every test below"""
    grads = gb.lattice_grads(0)
    return dict(grads=grads, ref=gb.reference(grads), allowed=gb.budget(grads), stats=gb.model_stats(grads))


def ratios(stats, ref, allowed):
    """worst error / budget per figure; the exact figures (absmax, count, total_inf) give 0 or inf"""
    rows, total, total_inf = ref
    arows, atotal = allowed
    return dict(l2=gb.worst(stats["rows"][:, 0], rows[:, 0], arows[:, 0]), absmax=gb.worst(stats["rows"][:, 1], rows[:, 1], arows[:, 1]),
                absmean=gb.worst(stats["rows"][:, 2], rows[:, 2], arows[:, 2]), nonfinite=gb.worst(stats["rows"][:, 3], rows[:, 3], arows[:, 3]),
                total_l2=gb.worst(stats["total_l2"], total, atotal), total_inf=gb.worst(stats["total_inf"], total_inf, 0.0))


def bits_equal(a, b):
    return all(np.array_equal(np.asarray(x, dtype=F).view(np.int32), np.asarray(y, dtype=F).view(np.int32)) for x, y in zip(a, b))


def torch_clip(grads, max_norm, norm_type=2.0, foreach=None):
    params = [torch.nn.Parameter(torch.zeros(g.size)) for g in grads]
    for p, g in zip(params, grads):
        p.grad = torch.from_numpy(g.copy())
    total = torch.nn.utils.clip_grad_norm_(params, max_norm, norm_type, foreach=foreach)
    return F(total.item()), [p.grad.numpy() for p in params]


# ---------------------------------------------------------------------------------------------------------------- the model
def test_model_stays_inside_every_budget(lattice):
    r = ratios(lattice["stats"], lattice["ref"], lattice["allowed"])
    print(f"numpy model of the kernels' order: worst error / budget {({k: round(v, 3) for k, v in r.items()})}")
    assert max(r.values()) < 1, r
    # torch's CPU result, for the record, in units of the budget (fp32 accumulation: tens of ulp; not asserted)
    ref_total, atotal = lattice["ref"][1], lattice["allowed"][1]
    for foreach in (False, True):
        t, _ = torch_clip(lattice["grads"], 1e9, foreach=foreach)
        print(f"torch.nn.utils.clip_grad_norm_ (CPU, foreach={foreach}): total {t!r}, error / budget {abs(float(t) - ref_total) / atotal:.1f}")
    per = [abs(float(torch.from_numpy(g).norm()) - lattice["ref"][0][k, 0]) / lattice["allowed"][0][k, 0] for k, g in enumerate(lattice["grads"])]
    print(f"torch g.norm() per tensor (CPU): worst error / budget {max(per):.1f}")


@pytest.mark.parametrize("norm_type", [2.0, INF])
@pytest.mark.parametrize("where", ["below", "near", "above"])
def test_model_clip_is_the_fp32_formula(lattice, norm_type, where):
    stats = lattice["stats"]
    total = stats["total_inf"] if norm_type == INF else stats["total_l2"]
    max_norm = {"below": 0.25 * float(total), "near": float(np.nextafter(total, F(0))), "above": 1e6 * float(total)}[where]
    coef, out = gb.model_clip(stats, max_norm, norm_type)
    assert coef.dtype == F and coef.tobytes() == gb.clip_coef(max_norm, total).tobytes()
    assert (coef < 1) == (where != "above")
    want = [g * coef for g in lattice["grads"]] if coef < 1 else lattice["grads"]
    assert bits_equal(out, want)


# ---------------------------------------------------------------------------------------------------------------- planted defects
def test_defect_fp32_accumulation_leaves_the_budget_on_the_589824_case():
    """589824 elements of +-0.7 (gb.constant_grads).  On random gradients the roundings of an fp32 chain in the kernels' tree order
    average out and stay inside the budget; with one magnitude every rounding of g^2 and of the 16 additions of a thread errs the same
    way, and the error shows: about 2.4 budgets on l2 and 2.9 on absmean, against 0.5 and 0 for the fp64 rule."""
    grads = gb.constant_grads()
    ref, allowed = gb.reference(grads), gb.budget(grads)
    good = ratios(gb.model_stats(grads, offsets=[0]), ref, allowed)
    bad = ratios(gb.model_stats(grads, offsets=[0], defect="fp32_accumulate"), ref, allowed)
    print(f"589824 x +-0.7: error / budget, fp64 rule {({k: round(v, 2) for k, v in good.items()})}, fp32 accumulation {({k: round(v, 2) for k, v in bad.items()})}")
    assert max(good.values()) < 1
    assert bad["l2"] > 1 and bad["absmean"] > 1 and bad["total_l2"] > 1


def test_defect_omitted_1e_6_shows_at_a_total_norm_of_order_1e_6():
    grads = [(np.random.default_rng(1).standard_normal(257) * 6e-8).astype(F)]
    stats = gb.model_stats(grads, offsets=[0])
    total = stats["total_l2"]
    assert 5e-7 < total < 2e-6
    max_norm = 0.5 * float(total)
    good, out = gb.model_clip(stats, max_norm)
    assert good.tobytes() == gb.clip_coef(max_norm, total).tobytes() and bits_equal(out, [grads[0] * good])
    bad, out_bad = gb.model_clip(stats, max_norm, defect="no_eps")
    assert bad.tobytes() != good.tobytes() and abs(float(bad) / float(good) - 1) > 0.3
    assert not bits_equal(out_bad, [grads[0] * good])


def test_defect_no_clamp_scales_gradients_that_are_inside_the_norm(lattice):
    stats = lattice["stats"]
    max_norm = 4.0 * float(stats["total_l2"])
    coef, out = gb.model_clip(stats, max_norm)
    assert coef == 1 and bits_equal(out, lattice["grads"])
    coef_bad, out_bad = gb.model_clip(stats, max_norm, defect="no_clamp")
    assert coef_bad > 1 and not bits_equal(out_bad, lattice["grads"])


@pytest.mark.parametrize("norm_type", [2.0, INF])
def test_defect_per_tensor_coefficient(lattice, norm_type):
    stats = lattice["stats"]
    total = stats["total_inf"] if norm_type == INF else stats["total_l2"]
    max_norm = 0.25 * float(total)
    coef, out = gb.model_clip(stats, max_norm, norm_type)
    want = [g * coef for g in lattice["grads"]]
    assert bits_equal(out, want)
    _, out_bad = gb.model_clip(stats, max_norm, norm_type, defect="per_tensor")
    # the small tensors lie inside max_norm on their own: a per-tensor coefficient leaves them unscaled
    assert bits_equal([out_bad[0]], [lattice["grads"][0]]) and not bits_equal(out_bad, want)


def test_defect_absmax_that_drops_a_nan():
    grads = gb.lattice_grads(2)
    grads[0][0] = np.nan                  # the first element
    grads[-1][-1] = np.inf                # the last element of the last chunk
    grads[3][2], grads[3][5] = -np.inf, np.inf
    stats = gb.model_stats(grads)
    rows = stats["rows"]
    assert np.isnan(rows[0, :3]).all() and rows[0, 3] == 1
    assert np.isinf(rows[-1, :3]).all() and rows[-1, 3] == 1
    assert np.isinf(rows[3, :3]).all() and rows[3, 3] == 2
    assert np.isnan(stats["total_l2"]) and np.isnan(stats["total_inf"]) and stats["found_inf"]
    ref = gb.reference(grads)[0]  # numpy's own rule is the same
    assert np.isnan(ref[0, :3]).all() and np.isinf(ref[-1, :3]).all()
    bad = gb.model_stats(grads, defect="drop_nan")
    assert not np.isnan(bad["rows"][0, 1]) and not np.isnan(bad["total_inf"])  # the defect: a finite maximum for a tensor with a NaN


def test_defect_statistics_of_the_scaled_gradients_in_the_fused_pass(lattice):
    scaled = [g * F(65536) for g in lattice["grads"]]
    fused = gb.model_stats(scaled, inv_scale=1.0 / 65536.0)
    assert bits_equal(fused["grads"], lattice["grads"]) and not fused["found_inf"]  # a power of two: the unscale is exact
    assert fused["rows"].tobytes() == lattice["stats"]["rows"].tobytes() and fused["total_l2"] == lattice["stats"]["total_l2"]
    assert max(ratios(fused, lattice["ref"], lattice["allowed"]).values()) < 1
    bad = gb.model_stats(scaled, inv_scale=1.0 / 65536.0, defect="stats_of_scaled")
    r = ratios(bad, lattice["ref"], lattice["allowed"])
    assert r["total_l2"] > 1e6 and r["absmax"] == INF, r


def test_defect_scale_pass_running_although_found_inf_is_set():
    grads = gb.lattice_grads(3)
    grads[-1][-1] = np.inf
    stats = gb.model_stats(grads, inv_scale=0.5)
    assert stats["found_inf"]
    coef, out = gb.model_clip(stats, 1.0, found_inf=True)
    assert bits_equal(out, stats["grads"])  # nothing stored: the gradients stay as the unscale pass left them
    _, out_bad = gb.model_clip(stats, 1.0, found_inf=True, defect="ignore_found_inf")
    assert not bits_equal(out_bad, stats["grads"])


# ---------------------------------------------------------------------------------------------------------------- exact arithmetic
def test_exact_arithmetic_case_reproduces_torch_bit_for_bit():
    grads = gb.exact_grads()
    assert sum(int(np.count_nonzero(g)) for g in grads) == 1385049 < 2 ** 24
    assert all(g[-1] == 1 for g in grads)
    stats = gb.model_stats(grads)
    assert stats["total_l2"] == F(1176.881103515625) == F(np.sqrt(1385049.0))
    assert np.array_equal(stats["rows"][:, 0], np.sqrt(np.array([np.count_nonzero(g) for g in grads], dtype=np.float64)).astype(F))
    for foreach in (False, True):
        t, _ = torch_clip(grads, 1e9, foreach=foreach)
        assert t == F(1176.881103515625), (foreach, t)
    coef, out = gb.model_clip(stats, 3.0)
    assert coef.tobytes() == (F(3.0) / (F(1176.881103515625) + F(1e-6))).tobytes()
    for foreach in (False, True):
        t, theirs = torch_clip(grads, 3.0, foreach=foreach)
        assert t == stats["total_l2"] and bits_equal(theirs, out) and bits_equal(theirs, [g * coef for g in grads])
    # and the inf norm
    coef_inf, out_inf = gb.model_clip(stats, 0.25, INF)
    t, theirs = torch_clip(grads, 0.25, INF)
    assert t == stats["total_inf"] == 1 and bits_equal(theirs, out_inf)


# ---------------------------------------------------------------------------------------------------------------- C-ABI
def test_c_abi_argument_errors_before_any_device_call(pkg, optim):
    """Every refusal returns on the host: the non-null 'device' addresses are never dereferenced, copied to or passed on."""
    lib = pkg._lib.load()
    err = lambda: lib.hh_last_error().decode()  # noqa: E731
    FAKE = 0x10000  # 16-byte aligned, never touched
    rows = np.zeros(3, dtype=optim._TENSOR)
    rows["grad"] = FAKE
    rows["numel"] = [17, 5000, 0]
    R = rows.ctypes.data
    table_need = lib.hh_optim_table_bytes(R, 3, 1)
    assert table_need == 3 * 56 + (1 + 2) * 8 + 56  # unchanged by this feature
    need = lib.hh_grad_stats_bytes(R, 3, 1)
    # totals, rows, per-tensor fp64 sums, one 24-byte record per chunk, first-chunk indices (padded to 8 bytes)
    assert need == 16 + 3 * 16 + 3 * 8 + 3 * 24 + 4 * 4
    assert lib.hh_grad_stats_bytes(None, 3, 1) == -1 and "hh_grad_stats_bytes: null" in err()
    assert lib.hh_grad_stats_bytes(R, -1, 1) == -1 and lib.hh_grad_stats_bytes(R, 3, 0) == -1
    assert lib.hh_grad_stats_bytes(None, 0, 1) == 16

    def stats(r=R, n=3, ng=1, inv=None, found=None, table=FAKE, tb=table_need, upload=1, work=FAKE, wb=need):
        return lib.hh_grad_stats(r, n, ng, inv, found, table, tb, upload, work, wb, None)

    def clip(r=R, n=3, ng=1, max_norm=1.0, norm=0, found=None, table=FAKE, tb=table_need, work=FAKE, wb=need):
        return lib.hh_grad_clip(r, n, ng, max_norm, norm, found, table, tb, work, wb, None)

    for fn, name in ((stats, "hh_grad_stats"), (clip, "hh_grad_clip")):
        assert fn(r=None) != 0 and err() == f"{name}: null tensor table"
        assert fn(table=None) != 0 and "null" in err()
        assert fn(work=None) != 0 and "null" in err()
        assert fn(table=FAKE + 4) != 0 and "aligned" in err()
        assert fn(work=FAKE + 8) != 0 and "aligned" in err()
        assert fn(n=-1) != 0 and fn(ng=0) != 0
        assert fn(tb=table_need - 1) != 0 and err() == f"{name}: table buffer too small (hh_optim_table_bytes)"
        assert fn(wb=need - 1) != 0 and err() == f"{name}: workspace too small (hh_grad_stats_bytes)"
        bad = rows.copy()
        bad["grad"][1] = 0
        assert fn(r=bad.ctypes.data) != 0 and err() == f"{name}: null gradient pointer in the tensor table"
        bad = rows.copy()
        bad["numel"][0] = -1
        assert fn(r=bad.ctypes.data) != 0 and "negative" in err()
        bad = rows.copy()
        bad["group"][1] = 1
        assert fn(r=bad.ctypes.data) != 0 and "group" in err()
    assert stats(upload=2) != 0 and stats(upload=3) != 0 and stats(upload=-1) != 0 and "upload" in err()
    assert stats(inv=FAKE) != 0 and "found_inf" in err()
    assert clip(max_norm=-1.0) != 0 and "max_norm" in err()
    assert clip(max_norm=float("nan")) != 0 and "max_norm" in err()
    assert clip(norm=2) != 0 and clip(norm=-1) != 0 and "norm type" in err()


# ---------------------------------------------------------------------------------------------------------------- Python
def test_python_refusals(optim):
    p = torch.nn.Parameter(torch.ones(4))
    p.grad = torch.ones(4)
    opt = torch.optim.SGD([p], lr=0.1)
    with pytest.raises(ValueError, match="norm_type"):
        optim.clip_grad_norm_(opt, 1.0, norm_type=3)
    with pytest.raises(ValueError, match="max_norm"):
        optim.clip_grad_norm_(opt, -1.0)
    with pytest.raises(ValueError, match="max_norm"):
        optim.clip_grad_norm_(opt, float("nan"))
    assert torch.equal(p.grad, torch.ones(4))  # refused before anything was scaled


@pytest.mark.parametrize("norm_type", [2.0, INF])
def test_any_other_optimizer_goes_through_torchs_function(optim, norm_type):
    grads = gb.lattice_grads(4)[:9]
    want_total, want = torch_clip(grads, 0.5, norm_type)
    params = [torch.nn.Parameter(torch.zeros(g.size)) for g in grads]
    for p, g in zip(params, grads):
        p.grad = torch.from_numpy(g.copy())
    extra = torch.nn.Parameter(torch.zeros(3))  # no gradient: not part of the norm
    opt = torch.optim.SGD([dict(params=params[:4]), dict(params=params[4:] + [extra])], lr=0.1)
    total = optim.clip_grad_norm_(opt, 0.5, norm_type)
    assert total.dim() == 0 and total.dtype == torch.float32 and F(total.item()) == want_total
    assert bits_equal([p.grad.numpy() for p in params], want) and extra.grad is None
    assert not optim.is_device_optimizer(opt)


def test_grad_stats_rows_maps_names_to_rows(optim):
    net = torch.nn.Sequential(torch.nn.Linear(3, 2), torch.nn.Linear(2, 1))
    named = list(net.named_parameters())
    params = [named[2][1], named[0][1], named[3][1]]  # table order differs from the module's; one parameter has no row
    assert optim.grad_stats_rows(named, params) == {"0.weight": 1, "1.weight": 0, "1.bias": 2}
    assert (optim.STAT_L2, optim.STAT_ABSMAX, optim.STAT_ABSMEAN, optim.STAT_NONFINITE) == (0, 1, 2, 3)
