"""-m gpu: the weight EMA (csrc/ema.hip) through optim.ModelEMA, the modules and the C-ABI, against the fp64 reference and the derived
budget of tests/ema_budget.py.

1. Lattice through optim.Adam / AdamW / SGD with an attached ModelEMA: tensors of 1 .. 65539 elements, all pointers 16-byte aligned /
   the average alone one float off / the parameter alone one float off, n_averaged 0, 1, 7, 10^6, decay 0.9998, 0.5, 0, 1, warm-up off
   and on.  (a) p, state and step bits are those of the step without an EMA, (b) the average is inside the budget, (c) fused = step
   followed by the stand-alone update, bit for bit, (d) a second run gives the same bits, (e) the sentinels around every buffer stay.
2. n == 0 copies bits (-0.0 and a denormal among them).  3. A step skipped on found_inf keeps average and counter, fused and stand-alone,
   and the next clean step updates as if it had not happened.  4. Swap: once exchanges, twice restores; the engine sees it.
5. A thousand tensors of 1 .. 17 elements at odd offsets through the C-ABI, with EMA-only rows and NULL-average rows, and every refusal.
6. KeypointsModule / ClassificationModule with ema_decay.  7. torch.optim.Adam + ema.update() against AveragedModel.
8. load_checkpoint(use_ema=True).
"""
import copy
import importlib

import numpy as np
import pytest
import torch

import ema_budget as eb
import optim_budget as ob
from conftest import PKG

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = [1, 3, 4, 5, 255, 4095, 4096, 4097, 8195, 65539]
SENTINEL = 12345.0
GUARD = 8
STEP0 = 7
HYPER = {"Adam": dict(lr=1e-3, weight_decay=1e-2), "AdamW": dict(lr=1e-3, weight_decay=1e-2),
         "SGD": dict(lr=0.05, weight_decay=1e-4, momentum=0.9, nesterov=True)}


@pytest.fixture(scope="module")
def optim():
    return importlib.import_module(PKG + ".optim")


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


def _layout(sizes, off):
    """-> (start of each tensor in a flat buffer, total): every tensor `off` floats past a 16-byte boundary, GUARD sentinels apart"""
    starts, cur = [], 0
    for n in sizes:
        cur = (cur + GUARD + 3) // 4 * 4 + off
        starts.append(cur)
        cur += n
    return starts, cur + GUARD


class Flat:
    """arrays laid out in one device buffer of sentinels"""

    def __init__(self, arrays, off):
        self.starts, total = _layout([len(a) for a in arrays], off)
        host = np.full(total, SENTINEL, dtype=np.float32)
        self.inside = np.zeros(total, dtype=bool)
        for s, a in zip(self.starts, arrays):
            host[s:s + len(a)] = a
            self.inside[s:s + len(a)] = True
        self.buf = torch.from_numpy(host).to(DEV)
        self.views = [self.buf[s:s + len(a)] for s, a in zip(self.starts, arrays)]
        assert all(v.data_ptr() % 16 == 4 * off for v in self.views)

    def intact(self):
        return bool((self.buf.cpu().numpy()[~self.inside] == SENTINEL).all())

    def bits(self):
        """the tensors' elements in order, without the sentinels"""
        return _bits(self.buf)[torch.from_numpy(self.inside)]


class Bag(torch.nn.Module):
    def __init__(self, params):
        super().__init__()
        self.ps = torch.nn.ParameterList(params)


_HOST = {}


def _host_operands():
    """fp32 p, g, m, v and an earlier average per lattice tensor (made once)"""
    if not _HOST:
        scale = (1e-6, 1e-3, 1.0, 30.0)
        ops = []
        for k, n in enumerate(SIZES):
            p, g, m, v = ob.operands(300 + k, scale[k % 4], STEP0 + 1, n)
            rng = np.random.default_rng(900 + k)
            e = (p * (1 + 0.05 * rng.standard_normal(n)) + 1e-3 * rng.standard_normal(n)).astype(np.float32)
            ops.append((p, g, m, v, e))
        _HOST["ops"] = ops
    return _HOST["ops"]


class Setup:
    """The lattice tensors behind one optimizer and one ModelEMA (attached or not); align: "all", "ema" (the average alone one float
    past a 16-byte boundary) or "param" (the parameter alone)."""

    def __init__(self, optim, algo, align, n_avg, decay, warmup, attach, grads=None, params=None):
        ops = _host_operands()
        self.algo, self.n_avg, self.decay, self.warmup = algo, n_avg, decay, warmup
        self.host_e = [np.full_like(o[4], 777.0) if n_avg == 0 else o[4] for o in ops]  # (before the first update: anything)
        self.P = Flat(params if params is not None else [o[0] for o in ops], 1 if align == "param" else 0)
        self.G = Flat(grads if grads is not None else [o[1] for o in ops], 0)
        self.M = Flat([o[2] for o in ops], 0)
        self.V = Flat([o[3] for o in ops], 0)
        self.E = Flat(self.host_e, 1 if align == "ema" else 0)
        self.flats = (self.P, self.G, self.M, self.V, self.E)
        self.params = [torch.nn.Parameter(v) for v in self.P.views]
        for p, g in zip(self.params, self.G.views):
            p.grad = g
        self.bag = Bag(self.params)
        self.opt = getattr(optim, algo)(self.bag.parameters(), **HYPER[algo])
        for p, m, v in zip(self.params, self.M.views, self.V.views):
            if algo == "SGD":
                self.opt.state[p] = dict(momentum_buffer=m)
            else:
                self.opt.state[p] = dict(step=torch.tensor(float(STEP0), device=DEV), exp_avg=m, exp_avg_sq=v)
        self.ema = optim.ModelEMA(self.bag, self.opt if attach else None, decay=decay, warmup=warmup)
        for k, e in enumerate(self.E.views):
            self.ema.adopt_average(f"ps.{k}", e)
        self.ema.n_averaged.fill_(n_avg)

    def step_bits(self):
        """p, state and step counters"""
        out = [_bits(self.P.buf), _bits(self.M.buf)]
        if self.algo != "SGD":
            out += [_bits(self.V.buf), _bits(torch.stack([self.opt.state[p]["step"] for p in self.params]))]
        return out

    def ema_bits(self):
        return [_bits(self.E.buf), self.ema.n_averaged.cpu()]

    def intact(self):
        return all(f.intact() for f in self.flats)

    def worst(self, n_avg=None, before=None):
        """the averages against the fp64 rule applied to the parameters as the step left them"""
        n_avg = self.n_avg if n_avg is None else n_avg
        top = 0.0
        for k, (p, e) in enumerate(zip(self.P.views, self.E.views)):
            value, old = p.cpu().numpy(), (self.host_e if before is None else before)[k]
            top = max(top, eb.worst(e.cpu().numpy(), eb.ema_reference(old, value, n_avg, self.decay, self.warmup),
                                    eb.ema_budget(old, value, n_avg, self.decay, self.warmup)))
        return top


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


# ---------------------------------------------------------------------------------------------------------------- 1. the lattice
@pytest.mark.parametrize("align", ["all", "ema", "param"])
@pytest.mark.parametrize("algo", ["Adam", "AdamW", "SGD"])
def test_lattice_fused_step(optim, algo, align):
    top = 0.0
    for n_avg in eb.COUNTERS:
        for decay in eb.DECAYS:
            for warmup in eb.WARMUPS:
                case = (n_avg, decay, warmup)
                fused = Setup(optim, algo, align, n_avg, decay, warmup, attach=True)
                fused.opt.step()
                plain = Setup(optim, algo, align, n_avg, decay, warmup, attach=False)
                plain.opt.step()
                assert _same(fused.step_bits(), plain.step_bits()), case               # (a)
                assert _same(plain.ema_bits(), [_bits(Flat(plain.host_e, 1 if align == "ema" else 0).buf), torch.tensor(n_avg)]), case
                plain.ema.update()
                ratio = fused.worst()                                                  # (b)
                assert ratio <= 1, (case, ratio)
                top = max(top, ratio)
                assert _same(fused.ema_bits(), plain.ema_bits()), case                 # (c)
                assert int(fused.ema.n_averaged) == n_avg + 1, case
                if n_avg == 0:
                    assert torch.equal(fused.E.bits(), fused.P.bits()), case
                if n_avg and decay == 1.0:  # w = 0 without warm-up (with it the ramp, always below 1, is the decay): the average stays
                    assert warmup or torch.equal(_bits(fused.E.buf), _bits(Flat(fused.host_e, 1 if align == "ema" else 0).buf)), case
                again = Setup(optim, algo, align, n_avg, decay, warmup, attach=True)
                again.opt.step()
                assert _same(fused.step_bits() + fused.ema_bits(), again.step_bits() + again.ema_bits()), case  # (d)
                assert fused.intact() and plain.intact(), case                          # (e)
    print(f"{algo}, {align} aligned: worst average error / budget {top:.3f}")


def test_second_fused_step_reads_the_advanced_counter(optim):
    """two steps through one optimizer: the second runs at n + 1 (warm-up makes the weight depend on it) on the table the device holds"""
    s = Setup(optim, "Adam", "all", 1, 0.9998, True, attach=True)
    s.opt.step()
    assert s.worst() <= 1 and int(s.ema.n_averaged) == 2
    mid = [e.cpu().numpy().copy() for e in s.E.views]
    s.opt.step()
    assert s.worst(n_avg=2, before=mid) <= 1 and int(s.ema.n_averaged) == 3
    assert all(float(s.opt.state[p]["step"]) == STEP0 + 2 for p in s.params)
    assert s.intact()


def test_frozen_parameters_and_buffers_are_averaged_in_the_same_launch(optim):
    """a parameter without a gradient, a frozen one and (use_buffers) a float buffer are EMA-only rows; an integer buffer is not averaged"""
    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.a = torch.nn.Parameter(torch.randn(5000, device=DEV))
            self.idle = torch.nn.Parameter(torch.randn(33, device=DEV))
            self.frozen = torch.nn.Parameter(torch.randn(4099, device=DEV), requires_grad=False)
            self.register_buffer("running", torch.randn(17, device=DEV))
            self.register_buffer("count", torch.tensor(3, device=DEV))

    torch.manual_seed(0)
    for use_buffers in (False, True):
        net = Net()
        opt = optim.Adam([net.a, net.idle], lr=1e-2)
        ema = optim.ModelEMA(net, opt, decay=0.5, use_buffers=use_buffers)
        assert sorted(ema.averages) == sorted(["a", "idle", "frozen"] + (["running"] if use_buffers else []))
        net.a.grad = torch.randn_like(net.a)
        opt.step()  # n == 0: the copy
        with torch.no_grad():
            net.frozen.add_(1.0)
            net.idle.add_(1.0)
            net.running.add_(1.0)
            net.count.add_(1)
        before = {k: v.clone() for k, v in ema.averages.items()}
        opt.step()
        assert int(ema.n_averaged) == 2
        for name in ema.averages:
            value = getattr(net, name).detach().cpu().numpy()
            old = before[name].cpu().numpy()
            r = eb.worst(ema.averages[name].cpu().numpy(), eb.ema_reference(old, value, 1, 0.5, False), eb.ema_budget(old, value, 1, 0.5, False))
            assert r <= 1, (name, r)
            assert not torch.equal(before[name], ema.averages[name]), name
        sd = ema.state_dict()
        assert list(sd) == ["model", "n_averaged", "decay", "warmup", "use_buffers"]
        assert list(sd["model"]) == list(net.state_dict())
        assert sd["model"]["count"].item() == 4 and sd["model"]["count"].dtype == torch.int64  # copied when the state dict is made
        assert (sd["decay"], sd["warmup"], sd["use_buffers"]) == (0.5, False, use_buffers)
        assert sd["n_averaged"].dtype == torch.int64 and sd["n_averaged"].dim() == 0 and sd["n_averaged"].is_cuda
        if not use_buffers:
            assert torch.equal(sd["model"]["running"], net.running)  # the net's own, of the moment of the call
        fresh = optim.ModelEMA(Net(), None, decay=0.9, warmup=True, use_buffers=use_buffers)
        fresh.load_state_dict(copy.deepcopy(sd))
        assert (fresh.decay, fresh.warmup, int(fresh.n_averaged)) == (0.5, False, 2)
        assert all(torch.equal(_bits(fresh.averages[k]), _bits(ema.averages[k])) for k in ema.averages)
        with pytest.raises(ValueError, match="use_buffers"):
            optim.ModelEMA(Net(), None, use_buffers=not use_buffers).load_state_dict(sd)


# ---------------------------------------------------------------------------------------------------------------- 2. the copy
def test_first_update_copies_bits(optim):
    ops = _host_operands()
    params = [o[0].copy() for o in ops]
    for p in params[2:]:
        p[0], p[1] = -0.0, 1e-41  # a negative zero and a denormal
    s = Setup(optim, "SGD", "all", 0, 0.9998, True, attach=False, params=params)
    s.ema.update()
    got, want = s.E.bits(), s.P.bits()
    assert torch.equal(got, want) and int(s.ema.n_averaged) == 1
    assert (want == -2 ** 31).sum() >= len(params) - 2 and ((want > 0) & (want < 2 ** 23)).sum() >= len(params) - 2
    f = Setup(optim, "SGD", "ema", 0, 0.9998, True, attach=True, params=params)
    f.opt.step()
    assert torch.equal(f.E.bits(), f.P.bits()) and int(f.ema.n_averaged) == 1
    assert s.intact() and f.intact()


# ---------------------------------------------------------------------------------------------------------------- 3. the skip
@pytest.mark.parametrize("algo", ["Adam", "SGD"])
@pytest.mark.parametrize("where,value", [("last", float("inf")), ("first", float("nan"))])
def test_a_skipped_step_keeps_average_and_counter(optim, algo, where, value):
    ops = _host_operands()
    grads = [o[1].copy() for o in ops]
    if where == "last":
        grads[-1][-1] = value
    else:
        grads[0][0] = value
    for attach in (True, False):
        s = Setup(optim, algo, "all", 7, 0.5, False, attach=attach, grads=grads)
        found = torch.zeros((), device=DEV)
        s.opt.check_grads_nonfinite(found)
        assert found.item() == 1.0
        s.opt.grad_scale, s.opt.found_inf = torch.tensor(1.0, device=DEV), found
        before = s.step_bits() + s.ema_bits()
        s.opt.step()
        if not attach:
            s.ema.update(found_inf=found)
        assert _same(before, s.step_bits() + s.ema_bits()) and int(s.ema.n_averaged) == 7
        # the next, clean step: as if the skipped one had not happened
        for g, o in zip(s.G.views, ops):
            g.copy_(torch.from_numpy(o[1]))
        found.zero_()
        s.opt.check_grads_nonfinite(found)
        assert found.item() == 0.0
        s.opt.step()
        if not attach:
            s.ema.update(found_inf=found)
        clean = Setup(optim, algo, "all", 7, 0.5, False, attach=attach)
        clean.opt.step()
        if not attach:
            clean.ema.update()
        assert _same(s.step_bits() + s.ema_bits(), clean.step_bits() + clean.ema_bits()) and int(s.ema.n_averaged) == 8
        assert s.intact()


# ---------------------------------------------------------------------------------------------------------------- 4. the swap
@pytest.mark.parametrize("align", ["all", "ema", "param"])
def test_swap_exchanges_and_twice_restores(optim, align):
    s = Setup(optim, "Adam", align, 7, 0.5, False, attach=False)
    p0, e0 = s.P.bits(), s.E.bits()
    s.ema.swap()
    assert torch.equal(s.P.bits(), e0) and torch.equal(s.E.bits(), p0)
    s.ema.swap()
    assert torch.equal(s.P.bits(), p0) and torch.equal(s.E.bits(), e0)
    with s.ema.applied():
        assert torch.equal(s.P.bits(), e0)
    assert torch.equal(s.P.bits(), p0) and torch.equal(s.E.bits(), e0)
    assert s.intact() and int(s.ema.n_averaged) == 7


def _synth_net(pkg, seed=0):
    net = pkg.HigherHRNet(17, 32)
    net.load_state_dict({k: torch.from_numpy(pkg.synth.synth_param(k, v.shape, seed)) for k, v in net.state_dict().items()})
    return net.to(DEV)


def test_the_engine_sees_the_swap(pkg, optim):
    net = _synth_net(pkg).eval()
    ema = optim.ModelEMA(net, None, decay=0.5)
    ema.update()  # the copy
    with torch.no_grad():
        for p in net.parameters():
            p.mul_(1.02)
    net.mark_dirty()
    ema.update()  # now the average sits between the two
    x = torch.from_numpy(pkg.synth.synth_images(1, 32, 32, 0)).to(DEV)
    flat = lambda out: [t.clone() for t in out[0]] + [out[1].clone()]  # noqa: E731
    with torch.no_grad():
        own = flat(net(x))
        with ema.applied():
            averaged = flat(net(x))
        back = flat(net(x))
        other = pkg.HigherHRNet(17, 32).to(DEV).eval()
        other.load_state_dict(ema.state_dict()["model"])
        want = flat(other(x))
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(averaged, want))
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(own, back))
    assert not all(torch.equal(a, b) for a, b in zip(own, averaged))


# ---------------------------------------------------------------------------------------------------------------- 5. the C-ABI
class Arena:
    """n tensors of 1 .. 17 elements at odd element offsets in one buffer of sentinels"""

    def __init__(self, rng, n, scale=1.0, square=False):
        self.numel = 1 + np.arange(n) % 17
        self.starts, cur = np.zeros(n, dtype=np.int64), 0
        for i in range(n):
            cur += 1 + cur % 2  # a gap of one or two sentinels, and an odd start
            self.starts[i] = cur
            cur += self.numel[i]
        self.host = np.full(cur + 4, SENTINEL, dtype=np.float32)
        self.inside = np.zeros(cur + 4, dtype=bool)
        for s, m in zip(self.starts, self.numel):
            v = rng.standard_normal(m) * scale
            self.host[s:s + m] = v * v if square else v
            self.inside[s:s + m] = True
        self.dev = torch.from_numpy(self.host).to(DEV)

    def ptrs(self):
        return self.dev.data_ptr() + 4 * self.starts.astype(np.uint64)


def _abi_tables(optim, n, seed):
    rng = np.random.default_rng(seed)
    A = dict(p=Arena(rng, n), g=Arena(rng, n, 1e-2), m=Arena(rng, n, 1e-2), v=Arena(rng, n, 1e-2, square=True), e=Arena(rng, n))
    steps = torch.full((n,), 3.0, device=DEV)
    only_v = torch.from_numpy(rng.standard_normal(17 + 5000).astype(np.float32)).to(DEV)  # two EMA-only rows: 17 and 5000 elements
    only_e = torch.from_numpy(rng.standard_normal(17 + 5000).astype(np.float32)).to(DEV)
    rows = np.zeros(n, dtype=optim._TENSOR)
    for name, key in (("param", "p"), ("grad", "g"), ("state0", "m"), ("state1", "v")):
        rows[name] = A[key].ptrs()
    assert all(int(x) % 8 == 4 for x in rows["param"])
    rows["step"] = steps.data_ptr() + 4 * np.arange(n, dtype=np.uint64)
    rows["numel"] = A["p"].numel
    rows["group"] = 0
    groups = np.zeros(1, dtype=optim._GROUP)
    groups["lr"], groups["beta1"], groups["beta2"], groups["eps"] = 1e-3, 0.9, 0.999, 1e-8
    has = np.arange(n) % 10 != 3  # every tenth tensor has no average (row index -1)
    row_of = np.full(n, -1, dtype=np.int32)
    row_of[has] = 1 + np.arange(int(has.sum()))  # (row 0 and the last row are the EMA-only ones)
    erows = np.zeros(int(has.sum()) + 2, dtype=optim._EMA_ROW)
    erows["value"][1:-1], erows["ema"][1:-1], erows["numel"][1:-1] = A["p"].ptrs()[has], A["e"].ptrs()[has], A["p"].numel[has]
    erows["value"][0], erows["ema"][0], erows["numel"][0] = only_v.data_ptr(), only_e.data_ptr(), 17
    erows["value"][-1], erows["ema"][-1], erows["numel"][-1] = only_v.data_ptr() + 4 * 17, only_e.data_ptr() + 4 * 17, 5000
    return dict(A=A, steps=steps, only_v=only_v, only_e=only_e, rows=rows, groups=groups, row_of=row_of, erows=erows, has=has,
                n_avg=torch.tensor(5, dtype=torch.int64, device=DEV))


def _abi_bits(T):
    return [_bits(T["A"][k].dev) for k in "pgmve"] + [_bits(T["steps"]), _bits(T["only_v"]), _bits(T["only_e"]), T["n_avg"].cpu()]


def test_thousand_small_tensors_through_the_c_abi(pkg, optim):
    lib, n, decay = pkg._lib.load(), 1000, 0.9
    stream = torch.cuda.current_stream().cuda_stream
    F, P = _abi_tables(optim, n, 11), _abi_tables(optim, n, 11)  # fused; plain step + stand-alone update
    assert _same(_abi_bits(F), _abi_bits(P))
    nb = lib.hh_optim_table_bytes(F["rows"].ctypes.data, n, 1)
    ne = lib.hh_ema_table_bytes(F["erows"].ctypes.data, len(F["erows"]), n)
    assert ne == len(F["erows"]) * 24 + (len(F["erows"]) + 1) * 8 + n * 4
    tables = {k: torch.empty(nb, dtype=torch.uint8, device=DEV) for k in "FP"}
    etables = {k: torch.empty(ne, dtype=torch.uint8, device=DEV) for k in "FP"}

    def fused(T=F, **kw):
        a = dict(algo=optim.ALGO_ADAM, rows=T["rows"].ctypes.data, n=n, groups=T["groups"].ctypes.data, ngroups=1, scale=None, found=None,
                 table=tables["F"].data_ptr(), nb=nb, upload=optim.UPLOAD_ALL, erows=T["erows"].ctypes.data, nrows=len(T["erows"]),
                 row_of=T["row_of"].ctypes.data, decay=decay, warmup=0, n_avg=T["n_avg"].data_ptr(), etable=etables["F"].data_ptr(), ne=ne, eupload=1)
        a.update(kw)
        return lib.hh_optim_step_ema(a["algo"], a["rows"], a["n"], a["groups"], a["ngroups"], a["scale"], a["found"], a["table"], a["nb"], a["upload"],
                                     a["erows"], a["nrows"], a["row_of"], a["decay"], a["warmup"], a["n_avg"], a["etable"], a["ne"], a["eupload"], stream)

    # ---- every refusal returns non-zero and writes nothing
    before = _abi_bits(F)
    bad_rows, bad_erows, bad_of = F["rows"].copy(), F["erows"].copy(), F["row_of"].copy()
    bad_rows["numel"][5] = -1
    bad_erows["numel"][7] = -1
    mismatch = F["erows"].copy()
    mismatch["numel"][1] += 1
    null_e = F["erows"].copy()
    null_e["ema"][3] = 0
    high, low, twice = bad_of.copy(), bad_of.copy(), bad_of.copy()
    high[0], low[1], twice[1] = len(F["erows"]), -2, twice[0]
    refusals = [dict(table=None), dict(etable=None), dict(groups=None), dict(erows=None), dict(row_of=None), dict(n_avg=None),
                dict(rows=bad_rows.ctypes.data), dict(erows=bad_erows.ctypes.data), dict(erows=mismatch.ctypes.data), dict(erows=null_e.ctypes.data),
                dict(decay=-1e-9), dict(decay=1.0 + 1e-9), dict(decay=float("nan")), dict(row_of=high.ctypes.data), dict(row_of=low.ctypes.data),
                dict(row_of=twice.ctypes.data), dict(table=tables["F"].data_ptr() + 8), dict(etable=etables["F"].data_ptr() + 8), dict(nb=nb - 1),
                dict(ne=ne - 1), dict(algo=3), dict(nrows=-1)]
    for kw in refusals:
        assert fused(**kw) != 0, kw
        assert lib.hh_last_error(), kw
    ue = lib.hh_ema_table_bytes(F["erows"].ctypes.data, len(F["erows"]), 0)
    alone = lambda rows=F["erows"], decay=decay, n_avg=F["n_avg"].data_ptr(), table=etables["F"].data_ptr(), nbytes=ue: lib.hh_ema_update(  # noqa: E731
        rows.ctypes.data, len(rows), decay, 0, n_avg, None, table, nbytes, 1, stream)
    assert alone(rows=bad_erows) != 0 and alone(decay=2.0) != 0 and alone(n_avg=None) != 0 and alone(table=None) != 0
    assert alone(table=etables["F"].data_ptr() + 4) != 0 and alone(nbytes=ue - 1) != 0 and alone(rows=null_e) != 0
    swap = lambda rows=F["erows"], table=etables["F"].data_ptr(), nbytes=ue: lib.hh_ema_swap(rows.ctypes.data, len(rows), table, nbytes, 1, stream)  # noqa: E731
    assert swap(rows=bad_erows) != 0 and swap(table=None) != 0 and swap(table=etables["F"].data_ptr() + 4) != 0 and swap(nbytes=ue - 1) != 0
    torch.cuda.synchronize()
    assert _same(before, _abi_bits(F))

    # ---- two steps: fused against plain step + stand-alone update, the second on the tables the device already holds
    for step, upload in ((1, 1), (2, 0)):
        old_e = F["A"]["e"].dev.cpu().numpy()
        old_only = F["only_e"].cpu().numpy()
        pkg._lib.check(fused(upload=optim.UPLOAD_ALL if upload else 0, eupload=upload))
        pkg._lib.check(lib.hh_optim_step(optim.ALGO_ADAM, P["rows"].ctypes.data, n, P["groups"].ctypes.data, 1, None, None, tables["P"].data_ptr(), nb,
                                         optim.UPLOAD_ALL if upload else 0, stream))
        pkg._lib.check(lib.hh_ema_update(P["erows"].ctypes.data, len(P["erows"]), decay, 0, P["n_avg"].data_ptr(), None, etables["P"].data_ptr(), ue,
                                         upload, stream))
        assert _same(_abi_bits(F), _abi_bits(P)), step
        assert int(F["n_avg"]) == 5 + step and torch.equal(F["steps"].cpu(), torch.full((n,), 3.0 + step))
        got_p, got_e = F["A"]["p"].dev.cpu().numpy(), F["A"]["e"].dev.cpu().numpy()
        for k in "pgmve":  # the gaps
            arena = F["A"][k]
            assert (arena.dev.cpu().numpy()[~arena.inside] == SENTINEL).all(), k
        mask = np.zeros_like(F["A"]["e"].inside)
        for s, m, h in zip(F["A"]["e"].starts, F["A"]["e"].numel, F["has"]):
            mask[s:s + m] = h
        n_before = 5 + step - 1
        # (parameter and average arenas share one layout: the same random sizes, gaps and starts)
        assert np.array_equal(F["A"]["p"].starts, F["A"]["e"].starts)
        r = eb.worst(got_e[mask], eb.ema_reference(old_e[mask], got_p[mask], n_before, decay, False), eb.ema_budget(old_e[mask], got_p[mask], n_before, decay, False))
        assert r <= 1, (step, r)
        rest = F["A"]["e"].inside & ~mask  # tensors without an average: their slots in the arena stay as they were
        assert np.array_equal(got_e[rest].view(np.int32), old_e[rest].view(np.int32))
        only_v = F["only_v"].cpu().numpy()
        r = eb.worst(F["only_e"].cpu().numpy(), eb.ema_reference(old_only, only_v, n_before, decay, False), eb.ema_budget(old_only, only_v, n_before, decay, False))
        assert r <= 1, (step, r)
        assert not np.array_equal(F["only_e"].cpu().numpy(), old_only)
    # ---- swap through the C-ABI: twice is the identity
    before = _abi_bits(F)
    pkg._lib.check(swap())
    assert not _same(before, _abi_bits(F))
    assert torch.equal(_abi_bits(F)[6], before[7])  # the EMA-only values now hold the averages
    pkg._lib.check(swap())
    assert _same(before, _abi_bits(F))


# ---------------------------------------------------------------------------------------------------------------- 6. the modules
K, B, S = 17, 2, 128


def _keypoints_module(pkg, optim, precision, scale=None, ema_decay=0.5, ours=True):
    km = importlib.import_module(PKG + ".keypoints.model")
    net = pkg.HigherHRNet(K, 32)
    net.load_state_dict({k: torch.from_numpy(pkg.synth.synth_param(k, v.shape, 0)) for k, v in net.state_dict().items()})
    model = km.KeypointsModel(net)
    model.to_CUDA(0)
    model.net.train()
    opt = (optim.Adam if ours else torch.optim.Adam)(model.net.parameters(), lr=1e-3)
    module = km.KeypointsModule(model, pkg.AEKeypointsLoss(), opt, precision=precision, ema_decay=ema_decay)
    if precision == "fp16" and scale is not None:
        module.scalers["optim"] = type(module.scalers["optim"])("cuda", init_scale=scale)
    return module


@pytest.fixture(scope="module")
def batch(pkg):
    x = torch.from_numpy(pkg.synth.synth_images(B, S, S, 0))
    hms, masks, joints = pkg.synth.synth_train_targets(B, K, S, 3, seed=0)
    dev = lambda a: torch.tensor(a, device=DEV)  # noqa: E731
    return (x.to(DEV), [dev(h) for h in hms], [dev(m) for m in masks], joints)


def _flat(tensors):
    return torch.cat([t.detach().reshape(-1).cpu() for t in tensors])


def _averages(module):
    return _flat([module.ema.averages[name] for name, _ in module.model.net.named_parameters()])


def _three_steps_inside_the_chain_budget(module, batch, decay, steps=3):
    """after each step the averages against the fp64 chain formed from the parameters read back after that step: ref_k = rule(ref_k-1,
    p_k) in fp64, allowed_k = budget(ref_k-1, p_k) + (1 - w) allowed_k-1 (the update passes an earlier error on times 1 - w)"""
    ref = allowed = None
    for k in range(steps):
        module.training_step(batch, k)
        assert int(module.ema.n_averaged) == k + 1
        p, got = _flat(module.model.net.parameters()), _averages(module)
        if k == 0:
            assert torch.equal(got.view(torch.int32), p.view(torch.int32))  # the copy
            ref, allowed = p.double(), torch.zeros_like(p, dtype=torch.float64)
        else:
            w = eb.ema_weight(k, decay, False)
            allowed = eb.ema_budget(ref, p, k, decay, False) + (1.0 - w) * allowed
            ref = eb.ema_reference(ref, p, k, decay, False)
            ratio = eb.worst(got, ref, allowed)
            print(f"step {k + 1}: worst average error / chain budget {ratio:.3f}")
            assert ratio <= 1, (k, ratio)
            assert not torch.equal(got, p)


@pytest.fixture(scope="module")
def trained_bf16(pkg, optim, batch):
    module = _keypoints_module(pkg, optim, "bf16")
    assert module.ema.optimizer is module.optimizer  # attached: the fused launch
    _three_steps_inside_the_chain_budget(module, batch, 0.5)
    return module


def test_keypoints_module_bf16_average_inside_the_chain_budget(trained_bf16):
    assert int(trained_bf16.ema.n_averaged) == 3 and "ema" in trained_bf16.state_dict()


def test_keypoints_module_fp16_average_and_overflow(pkg, optim, batch):
    module = _keypoints_module(pkg, optim, "fp16", scale=1024.0)
    _three_steps_inside_the_chain_budget(module, batch, 0.5)
    assert module.scalers["optim"].get_scale() == 1024.0  # (all three steps were applied)
    # an overflowing step: average and counter stay
    module.scalers["optim"] = type(module.scalers["optim"])("cuda", init_scale=2.0 ** 40)
    before, p_before = _averages(module), _flat(module.model.net.parameters())
    module.training_step(batch, 3)
    assert module.scalers["optim"].get_scale() == 2.0 ** 39
    assert torch.equal(_averages(module).view(torch.int32), before.view(torch.int32)) and int(module.ema.n_averaged) == 3
    assert torch.equal(_flat(module.model.net.parameters()).view(torch.int32), p_before.view(torch.int32))


def test_keypoints_module_without_ema_is_the_step_as_before(pkg, optim, batch):
    module = _keypoints_module(pkg, optim, "bf16", ema_decay=None)
    assert module.ema is None and "ema" not in module.state_dict() and module.optimizer._ema is None


def test_module_state_dict_continues_with_the_same_bits(pkg, optim, batch, trained_bf16):
    a = trained_bf16
    b = _keypoints_module(pkg, optim, "bf16")
    b.model.load_state_dict(a.model.state_dict())
    b.optimizer.load_state_dict(copy.deepcopy(a.optimizer.state_dict()))
    b.load_state_dict(copy.deepcopy(a.state_dict()))
    assert int(b.ema.n_averaged) == int(a.ema.n_averaged) == 3
    assert torch.equal(_averages(a).view(torch.int32), _averages(b).view(torch.int32))
    # the same gradients into both (the gradients the last training step left): one optimizer step each
    for pa, pb in zip(a.model.net.parameters(), b.model.net.parameters()):
        pb.grad = pa.grad.clone()
    snapshot = (_flat(a.model.net.parameters()), _averages(a), a.ema.n_averaged.clone(), copy.deepcopy(a.optimizer.state_dict()))
    a.optimizer.step()
    b.optimizer.step()
    assert int(a.ema.n_averaged) == int(b.ema.n_averaged) == 4
    assert torch.equal(_flat(a.model.net.parameters()).view(torch.int32), _flat(b.model.net.parameters()).view(torch.int32))
    assert torch.equal(_averages(a).view(torch.int32), _averages(b).view(torch.int32))
    assert not torch.equal(_averages(a), snapshot[1])
    # (put the shared module back to its third step for the tests that follow)
    with torch.no_grad():
        for p, v in zip(a.model.net.parameters(), snapshot[0].split([p.numel() for p in a.model.net.parameters()])):
            p.copy_(v.view_as(p))
        for (name, _), v in zip(a.model.net.named_parameters(), snapshot[1].split([p.numel() for p in a.model.net.parameters()])):
            a.ema.averages[name].copy_(v.view_as(a.ema.averages[name]))
        a.ema.n_averaged.copy_(snapshot[2])
    a.optimizer.load_state_dict(snapshot[3])
    a.model.net.mark_dirty()


def test_validation_step_runs_on_the_averaged_weights(pkg, optim, batch, trained_bf16):
    km = importlib.import_module(PKG + ".keypoints.model")
    module = trained_bf16
    net = module.model.net
    weights = [_bits(p) for p in net.parameters()]
    net.eval()
    try:
        metrics, results = module.validation_step(batch)
    finally:
        net.train()
    assert all(torch.equal(w, _bits(p)) for w, p in zip(weights, net.parameters()))  # the training weights are back in place
    other = pkg.HigherHRNet(K, 32).to(DEV)
    other.load_state_dict(module.ema.state_dict()["model"])
    other.eval()
    plain = km.KeypointsModule(km.KeypointsModel(other), pkg.AEKeypointsLoss(), torch.optim.SGD(other.parameters(), lr=0.0))
    want, _ = plain.validation_step(batch)
    assert metrics == want, (metrics, want)
    own = pkg.HigherHRNet(K, 32).to(DEV)
    own.load_state_dict(net.state_dict())
    own.eval()
    last, _ = km.KeypointsModule(km.KeypointsModel(own), pkg.AEKeypointsLoss(), torch.optim.SGD(own.parameters(), lr=0.0)).validation_step(batch)
    assert last != metrics  # (and the last iterate gives something else)
    assert len(results) == B


def test_classification_module_with_ema(pkg, optim):
    cls = importlib.import_module(PKG + ".classification")
    torch.manual_seed(0)
    model = cls.ClassificationModel(pkg.ClassificationHRNet(32, 1000))
    model.init_weights()
    model.to_CUDA(0)
    model.net.train()
    opt = optim.SGD(model.net.parameters(), lr=0.01, momentum=0.9, nesterov=True, weight_decay=1e-4)
    module = cls.ClassificationModule(model, cls.ClassificationLoss(), opt, ema_decay=0.5, ema_use_buffers=True)
    batch = module.batch_to_device((torch.from_numpy(pkg.synth.synth_images(2, 64, 64, seed=2)), torch.tensor([3, 141])))
    names = [n for n, _ in model.net.named_parameters()]
    module.training_step(batch, 0)
    first = _flat([module.ema.averages[n] for n in names])
    assert torch.equal(first.view(torch.int32), _flat(model.net.parameters()).view(torch.int32))
    buffers = {n: b.detach().clone() for n, b in model.net.named_buffers() if b.is_floating_point()}
    assert buffers and all(torch.equal(_bits(module.ema.averages[n]), _bits(b)) for n, b in buffers.items())
    module.training_step(batch, 1)
    p, got = _flat(model.net.parameters()), _flat([module.ema.averages[n] for n in names])
    ratio = eb.worst(got, eb.ema_reference(first, p, 1, 0.5, False), eb.ema_budget(first, p, 1, 0.5, False))
    print(f"ClassificationModule: worst average error / budget {ratio:.3f}")
    assert ratio <= 1 and int(module.ema.n_averaged) == 2
    for n, old in buffers.items():  # the running statistics as the second forward left them, averaged with those of the first
        now = dict(model.net.named_buffers())[n].detach().cpu().numpy()
        r = eb.worst(module.ema.averages[n].cpu().numpy(), eb.ema_reference(old.cpu().numpy(), now, 1, 0.5, False),
                     eb.ema_budget(old.cpu().numpy(), now, 1, 0.5, False))
        assert r <= 1, (n, r)
    weights = [_bits(q) for q in model.net.parameters()]
    metrics, results = module.validation_step(batch)
    assert all(torch.equal(w, _bits(q)) for w, q in zip(weights, model.net.parameters())) and len(results) == 2
    sd = module.state_dict()
    assert list(sd) == ["ema"] and sd["ema"]["use_buffers"] is True and int(sd["ema"]["n_averaged"]) == 2


# ---------------------------------------------------------------------------------------------------------------- 7. stand-alone
def test_torch_adam_plus_update_against_averaged_model(optim):
    from torch.optim.swa_utils import AveragedModel, get_ema_multi_avg_fn
    decay = 0.9
    ops = _host_operands()
    bag = Bag([torch.nn.Parameter(torch.from_numpy(o[0]).to(DEV)) for o in ops])
    opt = torch.optim.Adam(bag.parameters(), lr=1e-2)
    ema = optim.ModelEMA(bag, opt, decay=decay)  # (not a device optimizer: nothing is attached)
    assert ema.optimizer is None
    theirs = AveragedModel(bag, multi_avg_fn=get_ema_multi_avg_fn(decay))
    ref = allowed = None
    for k in range(3):
        rng = np.random.default_rng(50 + k)
        for p in bag.parameters():
            p.grad = torch.from_numpy(rng.standard_normal(p.numel()).astype(np.float32)).to(DEV)
        opt.step()
        ema.update()
        theirs.update_parameters(bag)
        p = _flat(bag.parameters())
        ours, torchs = _flat([ema.averages[f"ps.{i}"] for i in range(len(ops))]), _flat(theirs.module.parameters())
        if k == 0:
            ref, allowed = p.double(), torch.zeros_like(p, dtype=torch.float64)
            assert torch.equal(ours.view(torch.int32), p.view(torch.int32)) and torch.equal(torchs.view(torch.int32), p.view(torch.int32))
        else:
            allowed = eb.ema_budget(ref, p, k, decay, False) + decay * allowed
            ref = eb.ema_reference(ref, p, k, decay, False)
            ro, rt = eb.worst(ours, ref, allowed), eb.worst(torchs, ref, allowed)
            rb = eb.worst(ours, torchs.double(), 2 * allowed)
            print(f"update {k + 1}: ModelEMA {ro:.3f}, AveragedModel {rt:.3f} of the budget; against each other {rb:.3f} of both")
            assert ro <= 1 and rt <= 1 and rb <= 1
    assert int(ema.n_averaged) == int(theirs.n_averaged) == 3


# ---------------------------------------------------------------------------------------------------------------- 8. checkpoints
def test_load_checkpoint_use_ema(pkg, trained_bf16, tmp_path):
    km = importlib.import_module(PKG + ".keypoints.model")
    module = trained_bf16
    path = str(tmp_path / "ckpt.pt")
    torch.save({"module": {**module.state_dict(), "model": module.model.state_dict()}}, path)
    infer = km.InferenceKeypointsModel(pkg.HigherHRNet(K, 32), device=DEV)
    infer.load_checkpoint(path, use_ema=True)
    loaded = dict(infer.net.named_parameters())
    assert all(torch.equal(_bits(loaded[n]), _bits(module.ema.averages[n])) for n, _ in module.model.net.named_parameters())
    infer.load_checkpoint(path)
    assert all(torch.equal(_bits(loaded[n]), _bits(p)) for n, p in module.model.net.named_parameters())
    torch.save({"module": {"scalers": {}, "model": module.model.state_dict()}}, path)
    with pytest.raises(KeyError, match="ema"):
        infer.load_checkpoint(path, use_ema=True)
    infer.load_checkpoint(path)
