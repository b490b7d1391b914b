"""-m gpu: gradient statistics and clipping by global norm (csrc/grad_stats.hip) through the C-ABI, through optim.clip_grad_norm_ /
optimizer.grad_stats() and through the modules, against the fp64 references and derived budgets of tests/grad_clip_budget.py.

1. Lattice: one table of tensors of 1 .. 4096 * 257 + 3 elements (the last takes the per-tensor reduction past one round of its
   workgroup), gradient scales 1e-6 .. 30, some gradients views into a flat buffer at offsets of 1 and 3 elements (the scalar path next
   to 16-byte chunks); max_norm below, near and far above the norm, both norm types.  Statistics inside their budgets, the coefficient
   and the clipped gradients bit for bit, a second run identical.  The exact-arithmetic case against torch on the device.  1000 tensors
   of 1 .. 40 elements through the raw C-ABI.
2. Loss scale: the fused unscale pass against hh_grads_nonfinite alone; a planted inf / NaN; the launches of one fp16 step.
3. Through the modules: KeypointsModule (bf16, fp16) and ClassificationModule against twins on torch.optim + torch's clip.
"""
import importlib

import numpy as np
import pytest
import torch

import grad_clip_budget as gb
import optim_budget as ob
from conftest import PKG

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32
INF = float("inf")
SENTINEL = 12345.0


@pytest.fixture(scope="module")
def optim():
    return importlib.import_module(PKG + ".optim")


def _dev(a):
    return torch.tensor(a, device=DEV)  # (always a copy: the host arrays stay the inputs)


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


def _same_bits(tensors, arrays):
    return all(np.array_equal(t.detach().cpu().numpy().view(np.int32), np.asarray(a, dtype=F).view(np.int32)) for t, a in zip(tensors, arrays))


class Table:
    """Parameters whose gradients are `grads`: tensor k's gradient is its own tensor (k % 3 == 0) or a view into `flat` at an element
    offset = 1 (k % 3 == 1) or 3 (k % 3 == 2) mod 4, with sentinel elements between the views (gb.OFFSETS)."""

    def __init__(self, optim, grads, algo="SGD", **hyp):
        self.host = [np.asarray(g, dtype=F) for g in grads]
        self.params = [torch.nn.Parameter(torch.full((g.size,), 0.5, device=DEV)) for g in self.host]
        total = sum(g.size + 8 for g in self.host)
        self.flat = torch.full((total,), SENTINEL, device=DEV)
        self.inside = torch.zeros(total, dtype=torch.bool)
        cur = 0
        for k, (g, p) in enumerate(zip(self.host, self.params)):
            if k % 3 == 0:
                p.grad = _dev(g)
                assert p.grad.data_ptr() % 16 == 0
            else:
                cur = (cur + 3) // 4 * 4 + gb.OFFSETS[k % 3]
                view = self.flat[cur:cur + g.size]
                view.copy_(_dev(g))
                self.inside[cur:cur + g.size] = True
                p.grad = view
                assert p.grad.data_ptr() % 16 in (4, 12)
                cur += g.size
        self.no_grad = torch.nn.Parameter(torch.arange(33, dtype=torch.float32, device=DEV))
        self.opt = getattr(optim, algo)(self.params + [self.no_grad], **(hyp or dict(lr=0.1)))

    def grads(self):
        return [p.grad for p in self.params]

    def sentinels_intact(self):
        return bool((self.flat.cpu()[~self.inside] == SENTINEL).all())


def _ratios(rows, total_l2, total_inf, grads):
    """worst error / budget per figure (rows: [n, 4] numpy fp32)"""
    ref_rows, ref_total, ref_inf = gb.reference(grads)
    arows, atotal = gb.budget(grads)
    r = {name: gb.worst(rows[:, c], ref_rows[:, c], arows[:, c]) for c, name in enumerate(("l2", "absmax", "absmean", "nonfinite"))}
    r["total_l2"], r["total_inf"] = gb.worst(total_l2, ref_total, atotal), gb.worst(total_inf, ref_inf, 0.0)
    return r


@pytest.fixture(scope="module")
def lattice_grads():
    return gb.lattice_grads(0)


@pytest.fixture(scope="module")
def lattice_model(lattice_grads):
    return gb.model_stats(lattice_grads)


# ---------------------------------------------------------------------------------------------------------------- lattice
@pytest.mark.parametrize("norm_type", [2.0, INF])
@pytest.mark.parametrize("where", ["below", "near", "above"])
def test_lattice_inside_the_budget_bit_exact_clip_and_repeatable(optim, lattice_grads, lattice_model, norm_type, where):
    grads = lattice_grads
    _, ref_l2, ref_inf = gb.reference(grads)
    ref_total = ref_inf if norm_type == INF else ref_l2
    # near: two fp32 steps under the norm (the budget lets the returned total sit one step from the reference's rounding), so that the
    # rounding of the sum with 1e-6 and of the division decide; the checks below take the coefficient from the RETURNED total
    near = np.nextafter(np.nextafter(F(ref_total), F(0)), F(0))
    max_norm = {"below": 0.25 * ref_total, "near": float(near), "above": 1e6 * ref_total}[where]
    runs = []
    for _ in range(2):
        t = Table(optim, grads)
        params, stats = t.opt.grad_stats()
        total = optim.clip_grad_norm_(t.opt, max_norm, norm_type)
        assert total.dim() == 0 and total.dtype == torch.float32 and total.is_cuda
        assert [id(p) for p in params] == [id(p) for p in t.params] and stats.shape == (len(grads), 4)
        runs.append((t, stats.cpu().numpy(), F(total.item()), F(t.opt.clip_coef().item())))
    t, rows, total, coef = runs[0]
    T = t.opt._rows
    totals = t.opt._totals(T).cpu().numpy()
    assert total.tobytes() == totals[1 if norm_type == INF else 0].tobytes()
    r = _ratios(rows, totals[0], totals[1], grads)
    print(f"lattice, norm {norm_type}, max_norm {where} ({max_norm:.6g}): total {total!r}, coef {coef!r}, worst error / budget "
          f"{({k: round(v, 3) for k, v in r.items()})}")
    assert max(r.values()) < 1, r
    # the figures are those of the host's model of the same summation order (test_grad_clip_cpu.py prints its ratios), bit for bit
    assert rows.tobytes() == lattice_model["rows"].tobytes()
    assert totals[0].tobytes() == lattice_model["total_l2"].tobytes() and totals[1].tobytes() == lattice_model["total_inf"].tobytes()
    assert coef.tobytes() == gb.clip_coef(max_norm, total).tobytes()  # the fp32 formula on the returned total, recomputed here
    assert (coef < 1) == (where != "above")
    want = [g * coef for g in grads] if coef < 1 else grads  # coef == 1: untouched
    assert _same_bits(t.grads(), want)
    assert t.sentinels_intact() and torch.equal(t.no_grad.detach().cpu(), torch.arange(33.0))
    t2, rows2, total2, coef2 = runs[1]
    assert rows.tobytes() == rows2.tobytes() and total.tobytes() == total2.tobytes() and coef.tobytes() == coef2.tobytes()
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(t.grads(), t2.grads()))


def test_constant_magnitude_case_inside_the_budget(optim):
    """589824 x +-0.7, where an fp32 accumulation leaves the budget (test_grad_clip_cpu.py): the kernel's fp64 rule does not"""
    grads = gb.constant_grads()
    t = Table(optim, grads)
    _, stats = t.opt.grad_stats()
    totals = t.opt._totals(t.opt._rows).cpu().numpy()
    r = _ratios(stats.cpu().numpy(), totals[0], totals[1], grads)
    print(f"589824 x +-0.7: worst error / budget {({k: round(v, 3) for k, v in r.items()})}")
    assert max(r.values()) < 1, r


def test_exact_arithmetic_case_equals_torch_on_the_device(optim):
    grads = gb.exact_grads()
    ours = Table(optim, grads)
    theirs = [torch.nn.Parameter(torch.zeros(g.size, device=DEV)) for g in grads]
    for p, g in zip(theirs, grads):
        p.grad = _dev(g)
    want = torch.nn.utils.clip_grad_norm_(theirs, 3.0)
    got = optim.clip_grad_norm_(ours.opt, 3.0)
    assert got.item() == want.item() == 1176.881103515625
    assert all(torch.equal(_bits(a), _bits(b.grad)) for a, b in zip(ours.grads(), theirs))
    assert F(ours.opt.clip_coef().item()).tobytes() == (F(3.0) / (F(1176.881103515625) + F(1e-6))).tobytes()
    assert ours.sentinels_intact()


def test_thousand_small_tensors_through_the_c_abi(pkg, optim):
    lib = pkg._lib.load()
    n = 1000
    sizes = 1 + np.arange(n) % 40
    starts = np.concatenate([[0], np.cumsum(sizes)[:-1]])  # packed: every alignment mod 4 occurs
    rng = np.random.default_rng(7)
    host = (rng.standard_normal(int(sizes.sum())) * 1e-2).astype(F)
    grads = [host[s:s + m] for s, m in zip(starts, sizes)]
    G = _dev(host)
    rows = np.zeros(n, dtype=optim._TENSOR)
    rows["grad"] = G.data_ptr() + 4 * starts.astype(np.uint64)
    rows["numel"] = sizes
    nbytes, wbytes = lib.hh_optim_table_bytes(rows.ctypes.data, n, 1), lib.hh_grad_stats_bytes(rows.ctypes.data, n, 1)
    assert nbytes == n * 56 + n * 8 + 56 and wbytes == 16 + n * (16 + 8 + 24 + 4)
    table = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    work = torch.full((wbytes,), 0xFF, dtype=torch.uint8, device=DEV)  # (nothing in it needs initialising)
    stream = torch.cuda.current_stream().cuda_stream
    pkg._lib.check(lib.hh_grad_stats(rows.ctypes.data, n, 1, None, None, table.data_ptr(), nbytes, optim.UPLOAD_TENSORS, work.data_ptr(), wbytes, stream))
    ref_total = gb.reference(grads)[1]
    max_norm = 0.5 * ref_total
    pkg._lib.check(lib.hh_grad_clip(rows.ctypes.data, n, 1, max_norm, optim.NORM_L2, None, table.data_ptr(), nbytes, work.data_ptr(), wbytes, stream))
    head = work[:16 + 16 * n].view(torch.float32).cpu().numpy()
    totals, got = head[:4], head[4:].reshape(n, 4)
    r = _ratios(got, totals[0], totals[1], grads)
    print(f"1000 tensors of 1 .. 40 elements: worst error / budget {({k: round(v, 3) for k, v in r.items()})}")
    assert max(r.values()) < 1, r
    coef = gb.clip_coef(max_norm, totals[0])
    assert totals[2].tobytes() == coef.tobytes() and coef < 1
    assert np.array_equal(G.cpu().numpy().view(np.int32), (host * coef).view(np.int32))


# ---------------------------------------------------------------------------------------------------------------- loss scale
def _count_launches(pkg, monkeypatch):
    """-> the list that receives the name of every entry point enqueued through _lib.launch, with its arguments"""
    log, real = [], pkg._lib.launch

    def launch(dev, fn, *args):
        log.append((fn.__name__, args))
        return real(dev, fn, *args)
    monkeypatch.setattr(pkg._lib, "launch", launch)
    return log


def test_fused_pass_at_loss_scale_65536(pkg, optim, lattice_grads, monkeypatch):
    log = _count_launches(pkg, monkeypatch)
    inv = torch.tensor(1.0 / 65536.0, device=DEV)
    fused, alone = Table(optim, lattice_grads), Table(optim, lattice_grads)
    for t in (fused, alone):
        for g in t.grads():
            g.mul_(65536.0)
    fused.opt.collect_grad_stats = True
    found_f, found_a = torch.zeros((), device=DEV), torch.zeros((), device=DEV)
    fused.opt.check_grads_nonfinite(found_f, inv)
    alone.opt.check_grads_nonfinite(found_a, inv)
    assert [name for name, _ in log] == ["hh_grad_stats", "hh_grads_nonfinite"]
    assert found_f.item() == found_a.item() == 0.0
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(fused.grads(), alone.grads()))
    assert _same_bits(fused.grads(), lattice_grads)  # a power of two: the unscale is exact
    assert fused.sentinels_intact() and alone.sentinels_intact()
    # the statistics: those of a separate call on the unscaled gradients, and no second read for them
    _, stats_f = fused.opt.grad_stats()
    assert len(log) == 2
    _, stats_a = alone.opt.grad_stats()
    assert [name for name, _ in log][2:] == ["hh_grad_stats"] and log[2][1][3] is None and log[2][1][4] is None
    assert torch.equal(_bits(stats_f), _bits(stats_a))
    assert torch.equal(_bits(fused.opt._totals(fused.opt._rows)[:2]), _bits(alone.opt._totals(alone.opt._rows)[:2]))
    # recompute=True reads again, and gives the same bits
    _, again = fused.opt.grad_stats(recompute=True)
    assert len(log) == 4 and torch.equal(_bits(again), _bits(stats_f))


@pytest.mark.parametrize("where,value", [("last", INF), ("first", float("nan"))])
def test_planted_non_finite_gradient(optim, lattice_grads, where, value):
    t = Table(optim, lattice_grads, "Adam", lr=1e-3)
    k, i = (len(lattice_grads) - 1, -1) if where == "last" else (0, 0)  # the last element of the last chunk / the first element
    with torch.no_grad():
        t.params[k].grad[i] = value
    t.opt.collect_grad_stats = True
    found = torch.zeros((), device=DEV)
    t.opt.check_grads_nonfinite(found, torch.tensor(0.5, device=DEV))
    assert found.item() == 1.0
    unscaled = [_bits(g) for g in t.grads()]
    _, stats = t.opt.grad_stats()
    total = optim.clip_grad_norm_(t.opt, 1e-3)
    rows = stats.cpu().numpy()
    bad = np.isnan if where == "first" else np.isinf
    assert bad(rows[k, :3]).all() and rows[k, 3] == 1 and bad(total.item())
    others = np.delete(np.arange(len(lattice_grads)), k)
    assert np.isfinite(rows[others]).all() and (rows[others, 3] == 0).all()
    halves = [g * F(0.5) for g in lattice_grads]
    r = _ratios(rows[others], 0.0, 0.0, [halves[j] for j in others])
    assert max(r["l2"], r["absmax"], r["absmean"]) < 1, r
    # the scale pass and the update store nothing
    before = [_bits(p) for p in t.params]
    t.opt.grad_scale, t.opt.found_inf = None, found
    t.opt.step()
    assert all(torch.equal(a, _bits(g)) for a, g in zip(unscaled, t.grads()))
    assert all(torch.equal(a, _bits(p)) for a, p in zip(before, t.params))
    for p in t.params:
        st = t.opt.state[p]
        assert float(st["step"]) == 0.0 and not st["exp_avg"].any() and not st["exp_avg_sq"].any()
    assert t.sentinels_intact()


def test_without_a_flag_a_non_finite_total_gives_torchs_gradients(optim):
    """no GradScaler in play (bf16): the coefficient is torch's 0 for an inf norm, and the gradients are torch's"""
    grads = gb.lattice_grads(5)[:9]
    grads[4][7] = np.inf
    ours = Table(optim, grads)
    theirs = [torch.nn.Parameter(torch.zeros(g.size, device=DEV)) for g in grads]
    for p, g in zip(theirs, grads):
        p.grad = _dev(g)
    want = torch.nn.utils.clip_grad_norm_(theirs, 1.0)
    got = optim.clip_grad_norm_(ours.opt, 1.0)
    assert got.item() == want.item() == INF and ours.opt.clip_coef().item() == 0.0
    assert all(torch.equal(_bits(a), _bits(b.grad)) for a, b in zip(ours.grads(), theirs))
    with pytest.raises(RuntimeError, match="non-finite"):
        optim.clip_grad_norm_(Table(optim, grads).opt, 1.0, error_if_nonfinite=True)


# ---------------------------------------------------------------------------------------------------------------- through the modules
K, B, S = 17, 2, 128
GRAD_CALLS = ("hh_grads_nonfinite", "hh_grad_stats", "hh_grad_clip", "hh_optim_step")  # the entry points that walk the gradient table


def _keypoints_module(pkg, optim, precision, ours, **kw):
    km = importlib.import_module(PKG + ".keypoints.model")
    net = pkg.HigherHRNet(K, 32)
    net.load_state_dict({k: torch.from_numpy(pkg.synth.synth_param(k, v.shape, 0)) for k, v in net.state_dict().items()})
    model = km.KeypointsModel(net)
    model.to_CUDA(0)
    model.net.train()
    opt = (optim.Adam if ours else torch.optim.Adam)(model.net.parameters(), lr=1e-3)
    module = km.KeypointsModule(model, pkg.AEKeypointsLoss(), opt, precision=precision, **kw)
    if precision == "fp16":  # a scale of 1024 keeps this batch's gradients finite, so the step is applied
        module.scalers["optim"] = type(module.scalers["optim"])("cuda", init_scale=1024.0)
    return module


@pytest.fixture(scope="module")
def batch(pkg):
    x = torch.from_numpy(pkg.synth.synth_images(B, S, S, 0))
    hms, masks, joints = pkg.synth.synth_train_targets(B, K, S, 3, seed=0)
    return (x.to(DEV), [_dev(h) for h in hms], [_dev(m) for m in masks], joints)


def _flat(tensors):
    return torch.cat([t.detach().reshape(-1).cpu() for t in tensors])


def _step(pkg, monkeypatch, module, where, batch):
    """one training step with the launches logged and the gradients copied as optim.clip_grad_norm_ receives them (after unscale_)
    -> dict(metrics, calls, g0, before)"""
    optim_mod = importlib.import_module(PKG + ".optim")
    mod = importlib.import_module(where)
    seen = {}

    def clip(optimizer, *a, **kw):
        seen["g0"] = [p.grad.detach().clone() for g in optimizer.param_groups for p in g["params"] if p.grad is not None]
        return optim_mod.clip_grad_norm_(optimizer, *a, **kw)
    log = _count_launches(pkg, monkeypatch)
    monkeypatch.setattr(mod, "clip_grad_norm_", clip)
    before = [p.detach().clone() for p in module.model.net.parameters()]
    metrics = module.training_step(batch, 0)
    monkeypatch.undo()
    return dict(metrics=metrics, calls=[(n, a) for n, a in log if n in GRAD_CALLS], g0=seen.get("g0"), before=before)


def _check_norm_and_clip(ours, theirs, ro, rt, max_norm, what):
    """the module checks shared by the three comparisons: equal losses, grad_norm against fp64 and against torch's, the coefficient
    and the clipped gradients bit for bit"""
    mo, mt = dict(ro["metrics"]), dict(rt["metrics"])
    no, nt = F(mo.pop("grad_norm")), F(mt.pop("grad_norm"))
    assert mo == mt, (mo, mt)
    go, gt = [g.cpu().numpy().ravel() for g in ro["g0"]], [g.cpu().numpy().ravel() for g in rt["g0"]]
    (_, ref_o, _), (_, ref_t, _) = gb.reference(go), gb.reference(gt)
    allowed = gb.budget(go)[1]
    torch_dev = abs(float(nt) - ref_t)
    print(f"{what}: grad_norm ours {no!r} torch {nt!r}; error / budget ours {abs(float(no) - ref_o) / allowed:.3f} torch {torch_dev / allowed:.1f}")
    assert abs(float(no) - ref_o) <= allowed
    assert abs(float(no) - float(nt)) <= allowed + torch_dev + abs(ref_o - ref_t)
    coef = F(ours.optimizer.clip_coef().item())
    assert coef.tobytes() == gb.clip_coef(max_norm, no).tobytes() and coef < 1
    params = list(ours.model.net.parameters())
    assert all(p.grad is not None for p in params) and len(go) == len(params)
    assert _same_bits([p.grad.reshape(-1) for p in params], [g * coef for g in go])
    return params


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_keypoints_module_clipped_step_against_torch(pkg, optim, batch, monkeypatch, precision):
    where, max_norm = PKG + ".keypoints.model", 1e-2
    theirs = _keypoints_module(pkg, optim, precision, False, max_grad_norm=max_norm)
    ours = _keypoints_module(pkg, optim, precision, True, max_grad_norm=max_norm)
    rt, ro = _step(pkg, monkeypatch, theirs, where, batch), _step(pkg, monkeypatch, ours, where, batch)
    params = _check_norm_and_clip(ours, theirs, ro, rt, max_norm, f"KeypointsModule {precision}")
    # the parameters: the existing Adam budget, evaluated on the clipped gradient left in .grad
    p0, g, p1 = _flat(ro["before"]), _flat([p.grad for p in params]), _flat(params)
    z = torch.zeros_like(p0)
    hyp = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=0.0, decoupled=False)
    ref, allowed = ob.adam_reference(p0, g, z, z, 1, **hyp), ob.adam_budget(p0, g, z, z, 1, **hyp)
    ratio = ob.worst(p1, ref[0], allowed[0])
    print(f"KeypointsModule {precision}: first clipped Adam step, worst error / budget {ratio:.3f}")
    assert ratio < 1
    assert {float(st["step"]) for st in ours.optimizer.state.values()} == {1.0}
    names = [n for n, _ in ro["calls"]]
    if precision == "bf16":
        assert names == ["hh_grad_stats", "hh_grad_clip", "hh_optim_step"]
        return
    # fp16, the launches that walk the gradients: the unscale launch is the statistics launch (1 read), the clip engaged (a 2nd)
    assert ours.scalers["optim"].get_scale() == theirs.scalers["optim"].get_scale() == 1024.0
    assert names == ["hh_grad_stats", "hh_grad_clip", "hh_optim_step"]
    stats_args = ro["calls"][0][1]
    assert stats_args[3] is not None and stats_args[4] is not None  # inv_scale and found_inf: the fused form
    assert ro["calls"][2][1][5] is None  # the update does not unscale again
    reads_before_update = 1 + int(ours.optimizer.clip_coef().item() < 1)
    assert reads_before_update == 2
    # a second step whose clip does not engage: one read before the update, the gradients exactly the unscaled ones
    ours.max_grad_norm = 1e9
    r2 = _step(pkg, monkeypatch, ours, where, batch)
    assert [n for n, _ in r2["calls"]] == ["hh_grad_stats", "hh_grad_clip", "hh_optim_step"]
    assert ours.optimizer.clip_coef().item() == 1.0  # every workgroup of the clip launch returned before reading a gradient
    assert all(torch.equal(_bits(p.grad), _bits(g)) for p, g in zip(ours.model.net.parameters(), r2["g0"]))
    assert np.isfinite(r2["metrics"]["grad_norm"]) and r2["metrics"]["grad_norm"] > 0


def test_classification_module_clipped_step_against_torch_sgd(pkg, optim, monkeypatch):
    cls = importlib.import_module(PKG + ".classification")
    where, max_norm = PKG + ".classification.module", 0.5
    hyp = dict(lr=0.01, momentum=0.9, nesterov=True, weight_decay=1e-4)
    modules = []
    for ours in (False, True):
        torch.manual_seed(0)
        model = cls.ClassificationModel(pkg.ClassificationHRNet(32, 1000))
        model.init_weights()
        model.to_CUDA(0)
        model.net.train()
        opt = (optim.SGD if ours else torch.optim.SGD)(model.net.parameters(), **hyp)
        modules.append(cls.ClassificationModule(model, cls.ClassificationLoss(), opt, max_grad_norm=max_norm))
    theirs, ours = modules
    batch = ours.batch_to_device((torch.from_numpy(pkg.synth.synth_images(2, 64, 64, seed=2)), torch.tensor([3, 141])))
    rt, ro = _step(pkg, monkeypatch, theirs, where, batch), _step(pkg, monkeypatch, ours, where, batch)
    params = _check_norm_and_clip(ours, theirs, ro, rt, max_norm, "ClassificationModule")
    p0, g, p1 = _flat(ro["before"]), _flat([p.grad for p in params]), _flat(params)
    z = torch.zeros_like(p0)
    bud = dict(lr=hyp["lr"], wd=hyp["weight_decay"], mu=hyp["momentum"], nesterov=True)
    ref, allowed = ob.sgd_reference(p0, g, z, **bud), ob.sgd_budget(p0, g, z, **bud)
    ratio = ob.worst(p1, ref[0], allowed[0])
    print(f"ClassificationModule: first clipped SGD step, worst error / budget {ratio:.3f}")
    assert ratio < 1
    assert [n for n, _ in ro["calls"]] == ["hh_grad_stats", "hh_grad_clip", "hh_optim_step"]


def test_max_grad_norm_none_is_the_module_without_the_argument(pkg, optim, batch, monkeypatch):
    km = PKG + ".keypoints.model"
    plain = _keypoints_module(pkg, optim, "fp16", True)
    none = _keypoints_module(pkg, optim, "fp16", True, max_grad_norm=None)
    rp, rn = _step(pkg, monkeypatch, plain, km, batch), _step(pkg, monkeypatch, none, km, batch)
    assert rp["metrics"] == rn["metrics"] and "grad_norm" not in rn["metrics"]
    assert rp["g0"] is None and rn["g0"] is None  # no clip call at all
    assert [n for n, _ in rp["calls"]] == [n for n, _ in rn["calls"]] == ["hh_grads_nonfinite", "hh_optim_step"]  # today's two launches
    assert not none.optimizer.collect_grad_stats
    for a, b in zip(plain.model.net.parameters(), none.model.net.parameters()):
        assert torch.equal(_bits(a), _bits(b)) and torch.equal(_bits(a.grad), _bits(b.grad))
    for pa, pb in zip(plain.model.net.parameters(), none.model.net.parameters()):
        sa, sb = plain.optimizer.state[pa], none.optimizer.state[pb]
        assert all(torch.equal(_bits(sa[k]), _bits(sb[k])) for k in ("step", "exp_avg", "exp_avg_sq"))


def test_grad_stats_rows_name_the_layers(pkg, optim):
    """the per-layer mean / max |grad| of the reference trainer's TODO, from one copy of the rows to the host"""
    net = torch.nn.Sequential(torch.nn.Linear(5, 3), torch.nn.Linear(3, 2)).to(DEV)
    opt = optim.SGD(net.parameters(), lr=0.1)
    net(torch.ones(4, 5, device=DEV)).sum().backward()
    params, stats = opt.grad_stats()
    rows = optim.grad_stats_rows(net.named_parameters(), params)
    assert list(rows) == ["0.weight", "0.bias", "1.weight", "1.bias"]
    host = stats.cpu().numpy()
    for name, p in net.named_parameters():
        g = p.grad.cpu().numpy().ravel()
        assert host[rows[name], optim.STAT_ABSMAX] == np.abs(g).max()
        assert abs(host[rows[name], optim.STAT_ABSMEAN] - np.abs(g.astype(np.float64)).mean()) <= 2 * gb.U * np.abs(g).mean() + 2.0 ** -150
