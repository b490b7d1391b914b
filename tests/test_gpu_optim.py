"""-m gpu: the device optimizer step (csrc/optim.hip) through the C-ABI and through pytorch-human-pose_amd/optim.py, against the fp64
references and derived budgets of tests/optim_budget.py.

1. Lattice: one table of tensors of 1 .. 589824 elements (the last two span several 4096-element chunks), some gradients views into a
   flat buffer at offsets of 1 and 3 elements (the scalar path next to float4 chunks), a parameter without a gradient and a frozen one,
   two param groups; per algorithm from injected state at step counters 0, 1, 999, 99999.  1000 tensors of 32 elements through the raw
   C-ABI (more descriptors than kernel arguments hold), twice, the second call on the table the device already holds.
2. Loss scale: grad_scale = 65536 equals the unscaled step bit for bit; one inf / one NaN sets the flag and the step stores nothing.
3. Through the modules: KeypointsModule (bf16, fp16 with the new scaler) and ClassificationModule against torch.optim on twin nets,
   a skipped fp16 step, state dicts crossing to torch.optim and back, create_optimizer.
"""
import importlib

import numpy as np
import pytest
import torch

import optim_budget as ob
from conftest import PKG

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = [1, 7, 8, 17, 255, 256, 257, 4096, 4097, 65539, 589824]
SENTINEL = 12345.0
ADAM_GROUPS = [dict(lr=1e-3, weight_decay=0.0), dict(lr=3e-3, weight_decay=1e-2)]
SGD_GROUPS = [dict(lr=0.05, weight_decay=1e-4, momentum=0.9, nesterov=True), dict(lr=0.01, weight_decay=0.0, momentum=0.0, nesterov=False)]
B1, B2, EPS = 0.9, 0.999, 1e-8


@pytest.fixture(scope="module")
def optim():
    return importlib.import_module(PKG + ".optim")


def _dev(a):
    return torch.tensor(a, device=DEV)  # (always a copy: the host arrays stay the step's inputs)


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


class Lattice:
    """The mixed table.  Tensor k belongs to group k % 2; its gradient is its own tensor (k % 3 == 0) or a view into `flat` at an
    element offset = 1 (k % 3 == 1) or 3 (k % 3 == 2) mod 4, with sentinel elements between the views."""

    def __init__(self, optim, algo, step0, grad_mul=1.0):
        self.algo, self.step0 = algo, step0
        adam = algo != "SGD"
        scale = (1e-6, 1e-3, 1.0, 30.0)
        self.host = []  # fp32 numpy operands per tensor: p, g, s0, s1
        for k, n in enumerate(SIZES):
            p, g, m, v = ob.operands(100 * k + step0 % 97, scale[k % 4], step0 + 1, n)
            if not adam:
                m = m * np.float32(10) if step0 else np.zeros_like(m)
            self.host.append((p, g, m, v))
        self.params = [torch.nn.Parameter(_dev(h[0])) for h in self.host]
        total = sum(n + 8 for n in SIZES)
        self.flat = torch.full((total,), SENTINEL, device=DEV)
        self.inside = torch.zeros(total, dtype=torch.bool)
        cur = 0
        for k, (n, p) in enumerate(zip(SIZES, self.params)):
            g = _dev(self.host[k][1]) * grad_mul
            if k % 3 == 0:
                p.grad = g
            else:
                cur = (cur + 3) // 4 * 4 + (1 if k % 3 == 1 else 3)
                view = self.flat[cur:cur + n]
                view.copy_(g)
                self.inside[cur:cur + n] = True
                p.grad = view
                assert p.grad.data_ptr() % 16 in (4, 12)
                cur += n
        self.no_grad = torch.nn.Parameter(torch.arange(33, dtype=torch.float32, device=DEV))
        self.frozen = torch.nn.Parameter(torch.arange(9, dtype=torch.float32, device=DEV), requires_grad=False)
        groups = [dict(params=self.params[0::2] + [self.no_grad], **(ADAM_GROUPS if adam else SGD_GROUPS)[0]),
                  dict(params=self.params[1::2] + [self.frozen], **(ADAM_GROUPS if adam else SGD_GROUPS)[1])]
        self.opt = getattr(optim, algo)(groups)
        for k, p in enumerate(self.params):
            _, _, m, v = self.host[k]
            if adam:
                self.opt.state[p] = dict(step=torch.tensor(float(step0), device=DEV), exp_avg=_dev(m),
                                         exp_avg_sq=_dev(v))
            elif step0 and SGD_GROUPS[k % 2]["momentum"]:
                self.opt.state[p] = dict(momentum_buffer=_dev(m))

    def state(self, k):
        st = self.opt.state[self.params[k]]
        return [st.get(key) for key in self.opt.STATE_KEYS]

    def check(self, applied=True):
        """every element of p and the state inside its budget (or, for a skipped step, bit-identical to the inputs); the counters"""
        adam = self.algo != "SGD"
        worst = {}
        for k, p in enumerate(self.params):
            hp, gp, m, v = self.host[k]
            got_p = p.detach().cpu().numpy()
            got_s = [None if s is None else s.cpu().numpy() for s in self.state(k)]
            if not applied:
                assert np.array_equal(got_p.view(np.int32), hp.view(np.int32)), k
                for got, want in zip(got_s, (m, v)):
                    assert got is None or np.array_equal(got.view(np.int32), want.view(np.int32)), k
            elif adam:
                hyp = dict(lr=ADAM_GROUPS[k % 2]["lr"], wd=ADAM_GROUPS[k % 2]["weight_decay"], b1=B1, b2=B2, eps=EPS, decoupled=self.algo == "AdamW")
                ref = ob.adam_reference(hp, gp, m, v, self.step0 + 1, **hyp)
                allowed = ob.adam_budget(hp, gp, m, v, self.step0 + 1, **hyp)
                for name, got, r, a in zip("pmv", [got_p] + got_s, ref, allowed):
                    worst[name] = max(worst.get(name, 0.0), ob.worst(got, r, a))
            else:
                g = SGD_GROUPS[k % 2]
                hyp = dict(lr=g["lr"], wd=g["weight_decay"], mu=g["momentum"], nesterov=g["nesterov"])
                ref, allowed = ob.sgd_reference(hp, gp, m, **hyp), ob.sgd_budget(hp, gp, m, **hyp)
                worst["p"] = max(worst.get("p", 0.0), ob.worst(got_p, ref[0], allowed[0]))
                if g["momentum"]:
                    worst["buf"] = max(worst.get("buf", 0.0), ob.worst(got_s[0], ref[1], allowed[1]))
                else:
                    assert "momentum_buffer" not in self.opt.state[p]
            if adam:
                assert float(self.opt.state[p]["step"]) == self.step0 + (1 if applied else 0), k
        assert torch.equal(self.no_grad.detach().cpu(), torch.arange(33.0)) and torch.equal(self.frozen.detach().cpu(), torch.arange(9.0))
        assert self.no_grad not in self.opt.state and self.frozen not in self.opt.state
        return worst

    def sentinels_intact(self):
        flat = self.flat.cpu()
        return bool((flat[~self.inside] == SENTINEL).all())

    def snapshot(self):
        out = [_bits(p) for p in self.params]
        for k in range(len(self.params)):
            out += [_bits(s) for s in self.state(k) if s is not None]
        return out


CASES = [(a, s) for a in ("Adam", "AdamW") for s in (0, 1, 999, 99999)] + [("SGD", 0), ("SGD", 1)]


@pytest.mark.parametrize("algo,step0", CASES)
def test_lattice_inside_the_budget_and_repeatable(optim, algo, step0):
    a = Lattice(optim, algo, step0)
    grads_before = [_bits(p.grad) for p in a.params]
    a.opt.step()
    worst = a.check()
    print(f"{algo} from step counter {step0}: worst error / budget {({k: round(v, 3) for k, v in worst.items()})}")
    assert max(worst.values()) < 1, worst
    assert a.sentinels_intact()
    assert all(torch.equal(x, _bits(p.grad)) for x, p in zip(grads_before, a.params))  # no scale: gradients are only read
    b = Lattice(optim, algo, step0)
    b.opt.step()
    assert all(torch.equal(x, y) for x, y in zip(a.snapshot(), b.snapshot()))


def test_second_step_reads_the_advanced_counters_and_a_scheduled_lr(optim):
    """two steps through the class with a MultiStepLR between them: the second runs at step counter + 2 and the new lr"""
    a = Lattice(optim, "Adam", 0)
    sched = torch.optim.lr_scheduler.MultiStepLR(a.opt, milestones=[1], gamma=0.1)
    a.opt.step()
    sched.step()
    assert a.opt.param_groups[0]["lr"] == pytest.approx(1e-4)
    mid = [(p.detach().cpu().numpy().copy(), *[s.cpu().numpy().copy() for s in a.state(k)]) for k, p in enumerate(a.params)]
    a.opt.step()
    for k, p in enumerate(a.params):
        p1, m1, v1 = mid[k]
        hyp = dict(lr=a.opt.param_groups[k % 2]["lr"], wd=ADAM_GROUPS[k % 2]["weight_decay"], b1=B1, b2=B2, eps=EPS, decoupled=False)
        g = a.host[k][1]
        ref, allowed = ob.adam_reference(p1, g, m1, v1, 2, **hyp), ob.adam_budget(p1, g, m1, v1, 2, **hyp)
        assert ob.worst(p.detach().cpu().numpy(), ref[0], allowed[0]) < 1, k
        assert float(a.opt.state[p]["step"]) == 2.0


def test_thousand_small_tensors_through_the_c_abi(pkg, optim):
    lib = pkg._lib.load()
    n, w = 1000, 32
    rng = np.random.default_rng(7)
    hp = (rng.standard_normal((n, w))).astype(np.float32)
    hg = (rng.standard_normal((n, w)) * 1e-2).astype(np.float32)
    hm, hv = np.zeros_like(hp), np.zeros_like(hp)
    P, Gr, M, V = [_dev(x) for x in (hp, hg, hm, hv)]
    steps = torch.zeros(n, device=DEV)
    rows = np.zeros(n, dtype=optim._TENSOR)
    for name, t in (("param", P), ("grad", Gr), ("state0", M), ("state1", V)):
        rows[name] = t.data_ptr() + 4 * w * np.arange(n, dtype=np.uint64)
    rows["step"] = steps.data_ptr() + 4 * np.arange(n, dtype=np.uint64)
    rows["numel"] = w
    rows["group"] = np.arange(n) % 2
    groups = np.zeros(2, dtype=optim._GROUP)
    groups["lr"], groups["weight_decay"] = [1e-3, 3e-3], [0.0, 1e-2]
    groups["beta1"], groups["beta2"], groups["eps"] = B1, B2, EPS
    nbytes = lib.hh_optim_table_bytes(rows.ctypes.data, n, 2)
    assert nbytes == n * 56 + n * 8 + 2 * 56
    table = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    for step, upload in ((1, optim.UPLOAD_ALL), (2, 0)):
        pkg._lib.check(lib.hh_optim_step(optim.ALGO_ADAM, rows.ctypes.data, n, groups.ctypes.data, 2, None, None, table.data_ptr(), nbytes, upload,
                                         stream))
        got = [t.cpu().numpy() for t in (P, M, V)]
        for gi in range(2):
            hyp = dict(lr=float(groups["lr"][gi]), wd=float(groups["weight_decay"][gi]), b1=B1, b2=B2, eps=EPS, decoupled=False)
            sel = slice(gi, None, 2)
            ref = ob.adam_reference(hp[sel], hg[sel], hm[sel], hv[sel], step, **hyp)
            allowed = ob.adam_budget(hp[sel], hg[sel], hm[sel], hv[sel], step, **hyp)
            for k in range(3):
                assert ob.worst(got[k][sel], ref[k], allowed[k]) < 1, (step, gi, k)
        assert torch.equal(steps.cpu(), torch.full((n,), float(step)))
        hp, hm, hv = got  # the next step starts from what this one stored


# ---------------------------------------------------------------------------------------------------------------- loss scale
@pytest.mark.parametrize("algo", ["Adam", "AdamW", "SGD"])
def test_grad_scale_65536_is_the_unscaled_step(optim, algo):
    plain = Lattice(optim, algo, 1)
    plain.opt.step()
    scaled = Lattice(optim, algo, 1, grad_mul=65536.0)
    scaled.opt.grad_scale = torch.tensor(65536.0, device=DEV)
    scaled.opt.found_inf = torch.zeros((), device=DEV)
    found = torch.zeros((), device=DEV)
    scaled.opt.check_grads_nonfinite(found)
    scaled.opt.step()
    assert found.item() == 0.0  # clean gradients leave the flag alone
    worst = scaled.check()
    assert max(worst.values()) < 1, worst
    assert all(torch.equal(x, y) for x, y in zip(plain.snapshot(), scaled.snapshot()))  # both divisions are exact for a power of two
    for ps, pp in zip(scaled.params, plain.params):  # the unscaled gradient is written back
        assert torch.equal(_bits(ps.grad), _bits(pp.grad))
    assert scaled.sentinels_intact()


def test_unscale_in_the_check_launch(optim):
    """GradScaler.unscale_'s form: the check multiplies by inv_scale in place; the views' surroundings stay"""
    a = Lattice(optim, "Adam", 1, grad_mul=1024.0)
    found = torch.zeros((), device=DEV)
    a.opt.check_grads_nonfinite(found, torch.tensor(1.0 / 1024.0, device=DEV))
    assert found.item() == 0.0 and a.sentinels_intact()
    for k, p in enumerate(a.params):
        assert np.array_equal(p.grad.cpu().numpy().view(np.int32), a.host[k][1].view(np.int32)), k


@pytest.mark.parametrize("algo", ["Adam", "SGD"])
@pytest.mark.parametrize("where,value", [("last", float("inf")), ("first", float("nan"))])
def test_a_non_finite_gradient_sets_the_flag_and_the_step_stores_nothing(optim, algo, where, value):
    a = Lattice(optim, algo, 1)
    with torch.no_grad():
        if where == "last":
            a.params[-1].grad[-1] = value
        else:
            a.params[0].grad[0] = value
    found = torch.zeros((), device=DEV)
    a.opt.check_grads_nonfinite(found)
    assert found.item() == 1.0
    a.opt.grad_scale, a.opt.found_inf = torch.tensor(4.0, device=DEV), found
    a.opt.step()
    a.check(applied=False)
    assert a.sentinels_intact()
    g = a.params[-1].grad if where == "last" else a.params[0].grad
    assert not torch.isfinite(g[-1] if where == "last" else g[0])  # and the gradients were not unscaled either


# ---------------------------------------------------------------------------------------------------------------- through the modules
K, B, S = 17, 2, 128


def _keypoints_module(pkg, optim, precision, ours, scale=None):
    km = importlib.import_module(PKG + ".keypoints.model")
    net = pkg.HigherHRNet(K, 32)
    net.load_state_dict({k: torch.from_numpy(pkg.synth.synth_param(k, v.shape, 0)) for k, v in net.state_dict().items()})
    model = km.KeypointsModel(net)
    model.to_CUDA(0)
    model.net.train()
    opt = (optim.Adam if ours else torch.optim.Adam)(model.net.parameters(), lr=1e-3)
    module = km.KeypointsModule(model, pkg.AEKeypointsLoss(), opt, precision=precision)
    if precision == "fp16":
        assert type(module.scalers["optim"]) is (optim.GradScaler if ours else torch.amp.GradScaler)
        if scale is not None:
            module.scalers["optim"] = type(module.scalers["optim"])("cuda", init_scale=scale)
    return module


@pytest.fixture(scope="module")
def batch(pkg):
    x = torch.from_numpy(pkg.synth.synth_images(B, S, S, 0))
    hms, masks, joints = pkg.synth.synth_train_targets(B, K, S, 3, seed=0)
    return (x.to(DEV), [_dev(h) for h in hms], [_dev(m) for m in masks], joints)


def _flat(tensors):
    return torch.cat([t.detach().reshape(-1).cpu() for t in tensors])


def _adam_first_step_ratio(before, params, lr=1e-3):
    """every parameter of a net after its first Adam step against the fp64 reference, from the gradients left in .grad"""
    p0, g, p1 = _flat(before), _flat([p.grad for p in params]), _flat(params)
    z = torch.zeros_like(p0)
    hyp = dict(lr=lr, b1=B1, b2=B2, eps=EPS, wd=0.0, decoupled=False)
    ref, allowed = ob.adam_reference(p0, g, z, z, 1, **hyp), ob.adam_budget(p0, g, z, z, 1, **hyp)
    return ob.worst(p1, ref[0], allowed[0])


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_keypoints_module_step_against_torch_adam(pkg, optim, batch, precision):
    # fp16: a scale of 1024 keeps this batch's gradients finite, so the step is applied (asserted below)
    theirs = _keypoints_module(pkg, optim, precision, False, scale=1024.0)
    ours = _keypoints_module(pkg, optim, precision, True, scale=1024.0)
    before = [p.detach().clone() for p in ours.model.net.parameters()]
    mt, mo = theirs.training_step(batch, 0), ours.training_step(batch, 0)
    assert mo == mt, (mo, mt)
    params = list(ours.model.net.parameters())
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in params)
    if precision == "fp16":
        assert ours.scalers["optim"].get_scale() == theirs.scalers["optim"].get_scale() == 1024.0
        assert ours.state_dict() == theirs.state_dict()
    ratio = _adam_first_step_ratio(before, params)
    print(f"KeypointsModule {precision}: first Adam step, worst error / budget {ratio:.3f}")
    assert ratio < 1
    steps = {float(st["step"]) for st in ours.optimizer.state.values()}
    assert steps == {1.0} and len(ours.optimizer.state) == len(params)
    moved = sum(not torch.equal(b, p.detach()) for b, p in zip(before, params))
    assert moved > 0.9 * len(params), moved


def test_keypoints_module_fp16_overflow_is_skipped_by_both(pkg, optim, batch):
    theirs = _keypoints_module(pkg, optim, "fp16", False, scale=2.0 ** 40)
    ours = _keypoints_module(pkg, optim, "fp16", True, scale=2.0 ** 40)
    before = [p.detach().clone() for p in ours.model.net.parameters()]
    mt, mo = theirs.training_step(batch, 0), ours.training_step(batch, 0)
    assert mo == mt and np.isfinite(mo["loss"])
    for module in (theirs, ours):
        assert all(torch.equal(b, p.detach()) for b, p in zip(before, module.model.net.parameters()))
        assert module.scalers["optim"].get_scale() == 2.0 ** 39
    assert ours.state_dict() == theirs.state_dict()
    for st in ours.optimizer.state.values():
        assert float(st["step"]) == 0.0 and not st["exp_avg"].any() and not st["exp_avg_sq"].any()


def test_classification_module_step_against_torch_sgd(pkg, optim):
    cls = importlib.import_module(PKG + ".classification")
    hyp = dict(lr=0.01, momentum=0.9, nesterov=True, weight_decay=1e-4)
    modules = []
    for ours in (False, True):
        torch.manual_seed(0)
        model = cls.ClassificationModel(pkg.ClassificationHRNet(32, 1000))
        model.init_weights()
        model.to_CUDA(0)
        model.net.train()
        opt = (optim.SGD if ours else torch.optim.SGD)(model.net.parameters(), **hyp)
        modules.append(cls.ClassificationModule(model, cls.ClassificationLoss(), opt))
    theirs, ours = modules
    batch = ours.batch_to_device((torch.from_numpy(pkg.synth.synth_images(2, 64, 64, seed=2)), torch.tensor([3, 141])))
    before = [p.detach().clone() for p in ours.model.net.parameters()]
    assert all(torch.equal(a, b) for a, b in zip(before, theirs.model.net.parameters()))
    mt, mo = theirs.training_step(batch, 0), ours.training_step(batch, 0)
    assert mo == mt
    params = list(ours.model.net.parameters())
    p0, g, p1 = _flat(before), _flat([p.grad for p in params]), _flat(params)
    z = torch.zeros_like(p0)
    bud = dict(lr=hyp["lr"], wd=hyp["weight_decay"], mu=hyp["momentum"], nesterov=True)
    ref, allowed = ob.sgd_reference(p0, g, z, **bud), ob.sgd_budget(p0, g, z, **bud)
    buf = _flat([ours.optimizer.state[p]["momentum_buffer"] for p in params])
    rp, rb = ob.worst(p1, ref[0], allowed[0]), ob.worst(buf, ref[1], allowed[1])
    print(f"ClassificationModule: first SGD step, worst error / budget p {rp:.3f} momentum_buffer {rb:.3f}")
    assert rp < 1 and rb < 1


def test_state_dicts_cross_to_torch_and_back(optim):
    """ours -> torch.optim.Adam(capturable=True) -> ours, and the same for SGD: each continues from the other's state, ours inside budget"""
    rng = np.random.default_rng(3)
    hp, hg = rng.standard_normal(5000).astype(np.float32), (rng.standard_normal(5000) * 1e-2).astype(np.float32)
    hyp = dict(lr=1e-3, b1=B1, b2=B2, eps=EPS, wd=0.0, decoupled=False)

    def make(cls, **kw):
        p = torch.nn.Parameter(_dev(hp))
        p.grad = _dev(hg)
        return p, cls([p], **kw)

    def adam_step(p, opt, step, ours):
        st = opt.state[p]
        p0, m0, v0 = p.detach().cpu().numpy().copy(), st["exp_avg"].cpu().numpy().copy(), st["exp_avg_sq"].cpu().numpy().copy()
        opt.step()
        ref, allowed = ob.adam_reference(p0, hg, m0, v0, step, **hyp), ob.adam_budget(p0, hg, m0, v0, step, **hyp)
        got = (p.detach().cpu().numpy(), st["exp_avg"].cpu().numpy(), st["exp_avg_sq"].cpu().numpy())
        ratios = [ob.worst(got[k], ref[k], allowed[k]) for k in range(3)]
        print(f"{type(opt).__module__}.{type(opt).__name__} continues at step {step}: worst error / budget {[round(r, 3) for r in ratios]}")
        assert float(opt.state[p]["step"]) == step and not np.array_equal(got[0], p0)
        # the budget binds our kernel.  torch's capturable path forms 1 - beta^step from fp32 tensors (the planted defect "fp32 betas" of
        # test_optim_budget_cpu.py), so its own continuation is printed, and held to the moments' budgets, which that does not touch
        assert all(r < 1 for r in (ratios if ours else ratios[1:])), ratios

    p1, ours = make(optim.Adam, lr=1e-3)
    ours.step()
    sd = ours.state_dict()
    assert set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq"} and sd["state"][0]["step"].dtype == torch.float32
    p2, theirs = make(torch.optim.Adam, lr=1e-3, capturable=True)
    with torch.no_grad():
        p2.copy_(p1)
    theirs.load_state_dict(sd)
    adam_step(p2, theirs, 2, False)
    p3, back = make(optim.Adam, lr=1e-3)
    with torch.no_grad():
        p3.copy_(p2)
    back.load_state_dict(theirs.state_dict())
    adam_step(p3, back, 3, True)
    # SGD
    bud = dict(lr=0.05, wd=1e-4, mu=0.9, nesterov=True)
    kw = dict(lr=0.05, weight_decay=1e-4, momentum=0.9, nesterov=True)
    q1, a = make(optim.SGD, **kw)
    a.step()
    q2, b = make(torch.optim.SGD, **kw)
    with torch.no_grad():
        q2.copy_(q1)
    b.load_state_dict(a.state_dict())
    p0, b0 = q2.detach().cpu().numpy().copy(), b.state[q2]["momentum_buffer"].cpu().numpy().copy()
    b.step()
    ref, allowed = ob.sgd_reference(p0, hg, b0, **bud), ob.sgd_budget(p0, hg, b0, **bud)
    assert ob.worst(q2.detach().cpu().numpy(), ref[0], allowed[0]) < 1
    q3, c = make(optim.SGD, **kw)
    with torch.no_grad():
        q3.copy_(q2)
    c.load_state_dict(b.state_dict())
    p0, b0 = q3.detach().cpu().numpy().copy(), c.state[q3]["momentum_buffer"].cpu().numpy().copy()
    c.step()
    ref, allowed = ob.sgd_reference(p0, hg, b0, **bud), ob.sgd_budget(p0, hg, b0, **bud)
    assert ob.worst(q3.detach().cpu().numpy(), ref[0], allowed[0]) < 1
    assert ob.worst(c.state[q3]["momentum_buffer"].cpu().numpy(), ref[1], allowed[1]) < 1


def test_create_optimizer_maps_the_reference_names(optim):
    net = torch.nn.Linear(4, 3).to(DEV)
    net.bias.requires_grad = False
    for name, cls in (("Adam", optim.Adam), ("AdamW", optim.AdamW), ("SGD", optim.SGD), ("Adamax", torch.optim.Adamax),
                      ("Adadelta", torch.optim.Adadelta), ("Adagrad", torch.optim.Adagrad), ("RMSprop", torch.optim.RMSprop)):
        opt = optim.create_optimizer(net, name, lr=0.01)
        assert type(opt) is cls and [p for g in opt.param_groups for p in g["params"]] == [net.weight]
    with pytest.raises(ValueError, match="amsgrad"):
        optim.create_optimizer(net, "Adam", amsgrad=True)
    with pytest.raises(ValueError, match="sparse"):
        emb = torch.nn.Embedding(8, 4, sparse=True).to(DEV)
        opt = optim.SGD(emb.parameters(), lr=0.1)
        emb(torch.tensor([1, 2], device=DEV)).sum().backward()
        opt.step()
