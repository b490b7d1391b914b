"""The budgets of tests/optim_budget.py against torch's own CPU fp32 optimizers (they must pass) and against planted defects (each
must be flagged), the state-dict format, the constructor refusals and the C-ABI's argument errors.  No GPU needed."""
import importlib

import numpy as np
import pytest
import torch

import optim_budget as ob
from conftest import PKG

ADAM_HP = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8)


def _torch_adam(cls, p, g, m, v, step, wd):
    tp = torch.nn.Parameter(torch.from_numpy(p.copy()))
    tp.grad = torch.from_numpy(g.copy())
    opt = cls([tp], lr=ADAM_HP["lr"], betas=(ADAM_HP["b1"], ADAM_HP["b2"]), eps=ADAM_HP["eps"], weight_decay=wd, foreach=False)
    opt.state[tp] = dict(step=torch.tensor(float(step - 1)), exp_avg=torch.from_numpy(m.copy()), exp_avg_sq=torch.from_numpy(v.copy()))
    opt.step()
    st = opt.state[tp]
    assert float(st["step"]) == step
    return tp.detach().numpy(), st["exp_avg"].numpy(), st["exp_avg_sq"].numpy()


def _adam_cases():
    for si, step in enumerate(ob.STEPS):
        for gi, gs in enumerate(ob.GRAD_SCALES):
            for wd in ob.WDS:
                yield step, gs, wd, 1000 * si + 10 * gi


@pytest.mark.parametrize("decoupled", [False, True], ids=["adam", "adamw"])
def test_torch_cpu_adam_stays_inside_the_budget(decoupled):
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    w = [0.0, 0.0, 0.0]
    for step, gs, wd, seed in _adam_cases():
        p, g, m, v = ob.operands(seed, gs, step)
        got = _torch_adam(cls, p, g, m, v, step, wd)
        ref = ob.adam_reference(p, g, m, v, step, wd=wd, decoupled=decoupled, **ADAM_HP)
        allowed = ob.adam_budget(p, g, m, v, step, wd=wd, decoupled=decoupled, **ADAM_HP)
        for k in range(3):
            w[k] = max(w[k], ob.worst(got[k], ref[k], allowed[k]))
        # the op-by-op fp32 model of the kernel is held to the same budget
        emu = ob.adam_fp32(p, g, m, v, step, wd=wd, decoupled=decoupled, **ADAM_HP)
        for k in range(3):
            assert ob.worst(emu[k], ref[k], allowed[k]) < 1, (step, gs, wd, k)
    print(f"torch CPU {'AdamW' if decoupled else 'Adam'}: worst error / budget  p {w[0]:.3f}  m {w[1]:.3f}  v {w[2]:.3f}")
    assert max(w) < 1, w


SGD_CASES = [dict(lr=0.05, wd=1e-4, mu=0.9, nesterov=True), dict(lr=0.05, wd=1e-4, mu=0.9, nesterov=False), dict(lr=0.05, wd=0.0, mu=0.9, nesterov=True),
             dict(lr=0.01, wd=1e-2, mu=0.0, nesterov=False), dict(lr=0.01, wd=0.0, mu=0.0, nesterov=False)]


def _sgd_operands(seed, gs, fresh):
    p, g, m, _ = ob.operands(seed, gs, 10)
    return p, g, (np.zeros_like(m) if fresh else (m * np.float32(10)))


def test_torch_cpu_sgd_stays_inside_the_budget():
    w = [0.0, 0.0]
    for ci, hp in enumerate(SGD_CASES):
        for gi, gs in enumerate(ob.GRAD_SCALES):
            for fresh in (True, False):
                p, g, buf = _sgd_operands(50 * ci + gi, gs, fresh)
                tp = torch.nn.Parameter(torch.from_numpy(p.copy()))
                tp.grad = torch.from_numpy(g.copy())
                opt = torch.optim.SGD([tp], lr=hp["lr"], momentum=hp["mu"], weight_decay=hp["wd"], nesterov=hp["nesterov"], foreach=False)
                if hp["mu"] and not fresh:  # (fresh: torch's first step sets buf = g; the zero buffer of the reference gives the same)
                    opt.state[tp]["momentum_buffer"] = torch.from_numpy(buf.copy())
                opt.step()
                ref = ob.sgd_reference(p, g, buf, **hp)
                allowed = ob.sgd_budget(p, g, buf, **hp)
                emu = ob.sgd_fp32(p, g, buf, **hp)
                w[0] = max(w[0], ob.worst(tp.detach().numpy(), ref[0], allowed[0]))
                assert ob.worst(emu[0], ref[0], allowed[0]) < 1
                if hp["mu"]:
                    w[1] = max(w[1], ob.worst(opt.state[tp]["momentum_buffer"].numpy(), ref[1], allowed[1]))
                    assert ob.worst(emu[1], ref[1], allowed[1]) < 1
    print(f"torch CPU SGD: worst error / budget  p {w[0]:.3f}  momentum_buffer {w[1]:.3f}")
    assert max(w) < 1, w


@pytest.mark.parametrize("defect", ["no_bias_correction", "eps_in_root", "fp32_betas", "swap_decay"])
@pytest.mark.parametrize("decoupled", [False, True], ids=["adam", "adamw"])
def test_planted_adam_defects_are_flagged(defect, decoupled):
    flagged = []
    for step, gs, wd, seed in _adam_cases():
        p, g, m, v = ob.operands(seed, gs, step)
        ref = ob.adam_reference(p, g, m, v, step, wd=wd, decoupled=decoupled, **ADAM_HP)
        allowed = ob.adam_budget(p, g, m, v, step, wd=wd, decoupled=decoupled, **ADAM_HP)
        bad = ob.adam_fp32(p, g, m, v, step, wd=wd, decoupled=decoupled, defect=defect, **ADAM_HP)
        if max(ob.worst(bad[k], ref[k], allowed[k]) for k in range(3)) > 1:
            flagged.append((step, gs, wd))
    print(f"{defect}: flagged on {len(flagged)} lattice cases, e.g. {flagged[:3]}")
    assert flagged, defect


def test_plain_instead_of_nesterov_momentum_is_flagged():
    hp = SGD_CASES[0]
    flagged = 0
    for gi, gs in enumerate(ob.GRAD_SCALES):
        p, g, buf = _sgd_operands(gi, gs, False)
        ref, allowed = ob.sgd_reference(p, g, buf, **hp), ob.sgd_budget(p, g, buf, **hp)
        bad = ob.sgd_fp32(p, g, buf, defect="plain_momentum", **hp)
        flagged += ob.worst(bad[0], ref[0], allowed[0]) > 1
    assert flagged


def test_a_counter_advanced_on_a_skipped_step_is_flagged():
    """The counters' budget is equality.  One step late, the next applied step's bias corrections are those of step + 1: outside the
    parameter budget as well, at every early step of the lattice."""
    for step in (1, 2, 10):
        p, g, m, v = ob.operands(step, 1.0, step)
        ref = ob.adam_reference(p, g, m, v, step, wd=0.0, decoupled=False, **ADAM_HP)
        allowed = ob.adam_budget(p, g, m, v, step, wd=0.0, decoupled=False, **ADAM_HP)
        bad = ob.adam_fp32(p, g, m, v, step + 1, wd=0.0, decoupled=False, **ADAM_HP)
        assert ob.worst(bad[0], ref[0], allowed[0]) > 1, step
        assert float(step - 1) + 1 != float(step - 1)  # what the equality check on a skipped step's counter sees


# ---------------------------------------------------------------------------------------------------------------- classes, no GPU
@pytest.fixture(scope="module")
def optim():
    return importlib.import_module(PKG + ".optim")


def test_constructor_refusals(optim):
    cpu = [torch.nn.Parameter(torch.zeros(4))]
    for cls in (optim.Adam, optim.AdamW, optim.SGD):
        with pytest.raises(ValueError, match="on the GPU"):
            cls(cpu)
        with pytest.raises(ValueError, match="fp32"):
            cls([torch.nn.Parameter(torch.zeros(4, dtype=torch.float64))])
        with pytest.raises(ValueError, match="maximize"):
            cls(cpu, maximize=True)
        with pytest.raises(ValueError, match="differentiable"):
            cls(cpu, differentiable=True)
        with pytest.raises(ValueError):
            cls(cpu, lr=-1.0)
    for cls in (optim.Adam, optim.AdamW):
        with pytest.raises(ValueError, match="amsgrad"):
            cls(cpu, amsgrad=True)
        with pytest.raises(ValueError, match="beta"):
            cls(cpu, betas=(0.9, 1.0))
    with pytest.raises(ValueError, match="dampening"):
        optim.SGD(cpu, momentum=0.9, dampening=0.1)
    with pytest.raises(ValueError, match="Nesterov"):
        optim.SGD(cpu, nesterov=True)
    assert "grad_scaler" not in __import__("inspect").signature(optim.Adam.step).parameters
    assert optim.Adam._step_supports_amp_scaling and optim.SGD._step_supports_amp_scaling


def test_state_dict_format_round_trips_against_torch_on_cpu(optim):
    """As far as the format goes without a GPU: a state dict in the shape ours writes (fp32 0-dim `step` tensors, torch's keys) loads
    into torch's classes and steps, and what torch saves has the keys ours reads."""
    p = torch.nn.Parameter(torch.ones(5))
    for cls, keys in ((torch.optim.Adam, {"step", "exp_avg", "exp_avg_sq"}), (torch.optim.SGD, {"momentum_buffer"})):
        kw = dict(momentum=0.9) if cls is torch.optim.SGD else {}
        a = cls([p], lr=1e-3, **kw)
        p.grad = torch.full((5,), 0.5)
        a.step()
        sd = a.state_dict()
        assert set(sd["state"][0]) == keys
        state = {k: (v.clone().float().reshape(()) if k == "step" else v.clone()) for k, v in sd["state"][0].items()}
        b = cls([p], lr=1e-3, **kw)
        b.load_state_dict({"state": {0: state}, "param_groups": sd["param_groups"]})
        b.step()
        if "step" in keys:
            assert float(b.state[p]["step"]) == 2.0
    assert set(optim.optimizers) == {"Adam", "Adamax", "Adadelta", "Adagrad", "AdamW", "SGD", "RMSprop"}
    assert optim.optimizers["Adamax"] is torch.optim.Adamax and optim.optimizers["RMSprop"] is torch.optim.RMSprop
    assert optim.optimizers["Adadelta"] is torch.optim.Adadelta and optim.optimizers["Adagrad"] is torch.optim.Adagrad
    assert (optim.optimizers["Adam"], optim.optimizers["AdamW"], optim.optimizers["SGD"]) == (optim.Adam, optim.AdamW, optim.SGD)


# ---------------------------------------------------------------------------------------------------------------- C-ABI errors
def test_c_abi_argument_errors_before_any_device_call(pkg, optim):
    """Every refusal returns on the host: the non-null 'device' addresses are never dereferenced, copied to or passed on."""
    lib = pkg._lib.load()
    err = lambda: lib.hh_last_error().decode()  # noqa: E731
    FAKE = 0x10000  # 16-byte aligned, never touched
    rows = np.zeros(2, dtype=optim._TENSOR)
    for f in ("param", "grad", "state0", "state1", "step"):
        rows[f] = FAKE
    rows["numel"] = [17, 5000]
    groups = np.zeros(1, dtype=optim._GROUP)
    groups["lr"], groups["beta1"], groups["beta2"], groups["eps"] = 1e-3, 0.9, 0.999, 1e-8
    R, G = rows.ctypes.data, groups.ctypes.data
    need = lib.hh_optim_table_bytes(R, 2, 1)
    assert need == 2 * 56 + (1 + 2) * 8 + 56
    assert lib.hh_optim_table_bytes(None, 2, 1) == -1 and "null" in err()
    assert lib.hh_optim_table_bytes(R, -1, 1) == -1 and lib.hh_optim_table_bytes(R, 2, 0) == -1
    assert lib.hh_optim_table_bytes(None, 0, 1) == 56

    def step(algo=0, r=R, n=2, g=G, ng=1, table=FAKE, nbytes=need, upload=3):
        return lib.hh_optim_step(algo, r, n, g, ng, None, None, table, nbytes, upload, None)
    assert step(algo=3) != 0 and "algorithm" in err()
    assert step(algo=-1) != 0
    assert step(r=None) != 0 and "null" in err()
    assert step(g=None) != 0 and "null" in err()
    assert step(table=None) != 0 and "null" in err()
    assert step(table=FAKE + 4) != 0 and "aligned" in err()
    assert step(n=-1) != 0 and step(ng=0) != 0
    assert step(nbytes=need - 1) != 0 and "too small" in err()
    assert step(upload=4) != 0 and step(upload=-1) != 0
    for f in ("param", "grad", "state0", "state1", "step"):
        bad = rows.copy()
        bad[f][1] = 0
        assert step(r=bad.ctypes.data) != 0 and "null pointer" in err(), f
    bad = rows.copy()
    bad["numel"][0] = -1
    assert step(r=bad.ctypes.data) != 0 and "negative" in err()
    bad = rows.copy()
    bad["group"][1] = 1
    assert step(r=bad.ctypes.data) != 0 and "group" in err()
    badg = groups.copy()
    badg["beta2"] = 1.0
    assert step(g=badg.ctypes.data) != 0 and "beta" in err()
    # SGD: state1 / step may be NULL, state0 only where the group has no momentum
    sgd = rows.copy()
    sgd["state1"] = 0
    sgd["step"] = 0
    sgd["state0"] = 0
    mom = groups.copy()
    mom["momentum"] = 0.9
    assert step(algo=2, r=sgd.ctypes.data, g=mom.ctypes.data) != 0 and "null pointer" in err()
    # nothing to do is not an error, and launches nothing
    assert step(n=0, nbytes=56) == 0
    empty = rows.copy()
    empty["numel"] = 0
    assert step(r=empty.ctypes.data) == 0

    def check(r=R, n=2, ng=1, found=FAKE, table=FAKE, nbytes=need, upload=1):
        return lib.hh_grads_nonfinite(r, n, ng, None, found, table, nbytes, upload, None)
    assert check(found=None) != 0 and "null" in err()
    assert check(table=None) != 0 and check(r=None) != 0
    assert check(nbytes=need - 1) != 0 and "too small" in err()
    assert check(upload=2) != 0 and check(upload=3) != 0
    assert check(n=-1) != 0 and check(ng=0) != 0
    bad = rows.copy()
    bad["grad"][0] = 0
    assert check(r=bad.ctypes.data) != 0 and "null gradient" in err()
    assert check(n=0, nbytes=56) == 0
    assert lib.hh_abi_version() == 3
