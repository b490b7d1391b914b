"""-m "not gpu": the budget of tests/ema_budget.py holds an fp32 model of the EMA rule on every lattice case and catches each planted
defect on its named case; what ModelEMA, the checkpoint helper and the C-ABI refuse before they touch a device."""
import importlib

import numpy as np
import pytest
import torch

import ema_budget as eb
from conftest import PKG


@pytest.fixture(scope="module")
def optim():
    return importlib.import_module(PKG + ".optim")


def test_fp32_model_stays_inside_the_budget_on_the_whole_lattice():
    top = 0.0
    for seed, em, vm, n, decay, warmup in eb.cpu_cases():
        ema, value, old = eb.operands(seed, em, vm)
        got = eb.ema_fp32(ema, value, n, decay, warmup)
        ratio = eb.worst(got, eb.ema_reference(ema, value, n, decay, warmup), eb.ema_budget(ema, value, n, decay, warmup))
        assert ratio <= 1, (em, vm, n, decay, warmup, ratio)
        top = max(top, ratio)
    print(f"fp32 model over the CPU lattice: worst error / budget {top:.4f}")
    assert top > 0.5  # (the budget is not loose either: rounding to nearest reaches most of it)


def test_copy_and_skip_are_exact():
    ema, value, _ = eb.operands(1, 1.0, 1.0)
    value[0], value[1] = -0.0, 1e-41
    got = eb.ema_fp32(ema, value, 0, 0.9998, True)
    assert np.array_equal(got.view(np.int32), value.view(np.int32))
    assert not eb.ema_budget(ema, value, 0, 0.9998, True).any()
    got = eb.ema_fp32(ema, value, 7, 0.5, False, found_inf=True)
    assert np.array_equal(got.view(np.int32), ema.view(np.int32))
    assert not eb.ema_budget(ema, value, 7, 0.5, False, found_inf=True).any()


def test_warmup_ramp_and_weight():
    assert eb.ema_weight(1, 0.9998, True) == 1.0 - 2.0 / 11.0
    assert eb.ema_weight(10 ** 6, 0.9998, True) == 1.0 - 0.9998  # the ramp has passed the decay
    assert eb.ema_weight(1, 0.9998, False) == 1.0 - 0.9998
    assert eb.ema_weight(7, 0.0, True) == 1.0 and eb.ema_weight(7, 1.0, False) == 0.0


@pytest.mark.parametrize("defect", eb.DEFECTS)
def test_planted_defect_leaves_the_budget_on_its_named_case(defect):
    em, vm, n, decay, warmup, skip = eb.DEFECT_CASES[defect]
    ema, value, old = eb.operands(99, em, vm)
    ref, allowed = eb.ema_reference(ema, value, n, decay, warmup, skip), eb.ema_budget(ema, value, n, decay, warmup, skip)
    good = eb.worst(eb.ema_fp32(ema, value, n, decay, warmup, skip), ref, allowed)
    bad = eb.worst(eb.ema_fp32(ema, value, n, decay, warmup, skip, defect=defect, old_value=old), ref, allowed)
    print(f"{defect}: correct model {good:.3f}, defect {bad:.3g} of the budget")
    assert good <= 1 < bad


def test_budget_carries_the_error_of_an_fp64_chain_value():
    ema, value, _ = eb.operands(5, 1.0, 1.0)
    plain = eb.ema_budget(ema, value, 7, 0.5, False)
    chained = eb.ema_budget(ema, value, 7, 0.5, False, allowed_value=1e-6)
    assert np.allclose(chained - plain, 0.5 * 1e-6, rtol=1e-9, atol=0)
    assert np.all(eb.ema_budget(ema, value, 0, 0.5, False, allowed_value=1e-6) == 1e-6)


# ---- refusals that need no device
def test_model_ema_refuses_bad_arguments(optim):
    net = torch.nn.Linear(3, 2)
    for decay in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="decay"):
            optim.ModelEMA(net, decay=decay)
    with pytest.raises(ValueError, match="GPU"):
        optim.ModelEMA(net, decay=0.5)  # (host tensors: there is no CPU path)
    with pytest.raises(ValueError, match="fp32"):
        optim.ModelEMA(torch.nn.Linear(3, 2).double(), decay=0.5)
    with pytest.raises(ValueError, match="no parameters"):
        optim.ModelEMA(torch.nn.ReLU(), decay=0.5)


def test_checkpoint_weights_names_the_missing_ema_entry():
    km = importlib.import_module(PKG + ".keypoints.model")
    w, avg = {"a": torch.zeros(1)}, {"a": torch.ones(1)}
    assert km.checkpoint_weights({"module": {"model": w, "ema": {"model": avg}}}) is w
    assert km.checkpoint_weights({"module": {"model": w, "ema": {"model": avg}}}, use_ema=True) is avg
    assert km.checkpoint_weights(w) is w
    with pytest.raises(KeyError, match="ema"):
        km.checkpoint_weights({"module": {"model": w}}, use_ema=True)
    with pytest.raises(KeyError, match="module"):
        km.checkpoint_weights(w, use_ema=True)


def test_c_abi_refusals_come_before_any_device_work(pkg, optim):
    """every argument check of the entry points precedes their first HIP call, so they can be exercised without a GPU: the pointers
    below are never dereferenced"""
    lib = pkg._lib.load()
    rows = np.zeros(2, dtype=optim._EMA_ROW)
    rows["value"], rows["ema"], rows["numel"] = [4096, 8192], [12288, 16384], [5, 4097]
    assert lib.hh_ema_table_bytes(rows.ctypes.data, 2, 0) == 2 * 24 + 3 * 8
    assert lib.hh_ema_table_bytes(rows.ctypes.data, 2, 3) == 2 * 24 + 3 * 8 + 3 * 4
    assert lib.hh_ema_table_bytes(None, 0, 0) == 0
    bad = rows.copy()
    bad["numel"][1] = -1
    assert lib.hh_ema_table_bytes(bad.ctypes.data, 2, 0) == -1 and b"negative numel" in lib.hh_last_error()
    assert lib.hh_ema_table_bytes(None, 2, 0) == -1
    assert lib.hh_ema_table_bytes(rows.ctypes.data, 2, -1) == -1
    table, n_avg, nbytes = 1 << 20, 1 << 21, 72
    ok = dict(rows=rows.ctypes.data, nrows=2, decay=0.5, warmup=0, n=n_avg, found=None, table=table, nbytes=nbytes, upload=1)

    def update(**kw):
        a = {**ok, **kw}
        return lib.hh_ema_update(a["rows"], a["nrows"], a["decay"], a["warmup"], a["n"], a["found"], a["table"], a["nbytes"], a["upload"], None)

    for kw, word in ((dict(table=None), b"null"), (dict(table=table + 8), b"aligned"), (dict(nbytes=71), b"too small"), (dict(n=None), b"n_averaged"),
                     (dict(decay=-0.01), b"decay"), (dict(decay=1.01), b"decay"), (dict(decay=float("nan")), b"decay"),
                     (dict(rows=bad.ctypes.data), b"negative numel"), (dict(rows=None), b"null row table"), (dict(nrows=-1), b"nrows")):
        assert update(**kw) != 0, kw
        assert word in lib.hh_last_error(), (kw, lib.hh_last_error())
    assert lib.hh_ema_swap(rows.ctypes.data, 2, None, nbytes, 1, None) != 0
    assert lib.hh_ema_swap(rows.ctypes.data, 2, table, nbytes - 1, 1, None) != 0
    assert lib.hh_ema_swap(bad.ctypes.data, 2, table, nbytes, 1, None) != 0
